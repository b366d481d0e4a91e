// qp_sens.hip -- vector-Jacobian product of the batched QP solve (fsaempc_qp_vjp_batch_device).
//
// For a solved QP  min 1/2 x'Hx + g'x  s.t.  lb <= x <= ub, lbA <= A x <= ubA  with multipliers lambda (convention of the solver:
// H x + g - lambda_b - A' lambda_A = 0, >= 0 on a lower side, <= 0 on an upper side), the working set W is taken by the solver's own
// refinement rule (qp_solver.hip, "active-set refinement"): a side is in W iff its multiplier has the side's sign and exceeds the
// side's slack.  With A^ = [working rows; unit rows of the active bounds] the adjoint of the vertex map is, per cotangent column xbar,
//
//     H w + A^' mu = xbar,   A^ w = 0          =>   gbar = -w,  bbar_W = mu,  Hbar = -(w x' + x w')/2,  Abar_r = lambda_r w' - mu_r x'.
//
// One workgroup (4 waves) per instance.  Active bounds pin their variable (w = 0); on the free variables F, after a symmetric diagonal
// scaling (unit diagonal of H~, unit max-norm rows of A~):
//   M = H~_FF + rho A~_WF' A~_WF         fp64 MFMA SYRK over the working rows only (at most |F| of them), then Cholesky  M = L L'
//   Y = L^-1 A~_WF',  S = Y'Y            (S = A~ M^-1 A~', the dual operator of the augmented system), MFMA SYRK + Cholesky
// and each column is solved by the range-space formula on these two factors, followed by iterative refinement on the KKT residual of the
// adjoint system until it stagnates (<= 1e-12 relative or the instance reports status -1).  The multipliers of the pinned bounds
// follow from stationarity.  The factor M lives in LDS when n <= 128 (padded), otherwise in the instance's workspace slot, as do
// A~_WF, Y and S.  Every instance is computed by the same fixed sequence of operations on its own data only: results do not depend on
// the batch, the launch or the slot.
#include <hip/hip_runtime.h>
#include <math.h>
#include "qp_sens.h"

namespace {
typedef double v4d __attribute__((ext_vector_type(4)));
#define DEVINL __device__ __forceinline__

DEVINL int rup(int v, int a) { return (v + a - 1) / a * a; }
constexpr double RHO = 1.0;   // weight of A~'A~ in M (H~ has a unit diagonal, A~ unit rows)
constexpr int QPS_MAX_REFINE = 8;   // refinement passes at most (each: two triangular solves on M, two on S)

// max over the workgroup (NaN counts as +inf); red: >= 4 doubles of LDS
DEVINL double block_max(double v, double* red) {
  v = isnan(v) ? INFINITY : v;
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

// C[r + c ld] = base(r, c) + alpha (X'X)[r][c] on the lower 16 x 16 tiles (I >= J) of an Np x Np result; X row-major (K x Np, leading
// dimension ldx, rows Kp4 = K rounded up to 4, padding rows zero).  fp64 MFMA lane maps (qp_solver.hip): A[i=l&15][k=l>>4],
// B[k=l>>4][j=l&15], C/D col = l&15, row = (l>>4) + 4 reg.  Tiles are dealt round-robin to the 4 waves.
template <class Base>
DEVINL void syrk_lower(const double* X, int ldx, int Kp4, int Np, double* C, int ldc, double alpha, Base base) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int T = Np / 16;
  int t = 0;
  for (int I = 0; I < T; ++I)
    for (int J = 0; J <= I; ++J, ++t) {
      if ((t & 3) != wave) continue;
      v4d acc = {0.0, 0.0, 0.0, 0.0};
      const double* xa = X + (size_t)(lane >> 4) * ldx + 16 * I + (lane & 15);
      const double* xb = X + (size_t)(lane >> 4) * ldx + 16 * J + (lane & 15);
      for (int k0 = 0; k0 < Kp4; k0 += 4)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[(size_t)k0 * ldx], xb[(size_t)k0 * ldx], acc, 0, 0, 0);
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int r = 16 * I + (lane >> 4) + 4 * p, c = 16 * J + (lane & 15);
        C[r + (size_t)c * ldc] = base(r, c) + alpha * acc[p];
      }
    }
}

// In-place Cholesky of the leading nn x nn block (lower triangle read; on return L in the lower triangle and L' in the upper one, so
// that both triangular solves read contiguous columns).  false (uniform over the workgroup) on a non-positive pivot.
DEVINL bool cholesky(double* Mx, int ld, int nn) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int j = 0; j < nn; ++j) {
    __syncthreads();
    const double d = Mx[j + (size_t)j * ld];
    if (!(d > 0.0) || !isfinite(d)) { __syncthreads(); return false; }
    const double s = sqrt(d), si = 1.0 / s;
    for (int i = j + 1 + tid; i < nn; i += QPS_THREADS) {
      const double v = Mx[i + (size_t)j * ld] * si;
      Mx[i + (size_t)j * ld] = v; Mx[j + (size_t)i * ld] = v;
    }
    __syncthreads();
    if (tid == 0) Mx[j + (size_t)j * ld] = s;
    for (int c = j + 1 + wave; c < nn; c += 4) {
      const double lc = Mx[c + (size_t)j * ld];
      for (int i = c + lane; i < nn; i += 64) Mx[i + (size_t)c * ld] -= Mx[i + (size_t)j * ld] * lc;
    }
  }
  __syncthreads();
  return true;
}

// u = L^-1 v (v is overwritten); nn <= QPS_THREADS.  u, v in LDS.
DEVINL void solve_lower(const double* Mx, int ld, int nn, double* v, double* u) {
  const int tid = threadIdx.x;
  for (int j = 0; j < nn; ++j) {
    __syncthreads();
    const double uj = v[j] / Mx[j + (size_t)j * ld];
    if (tid == 0) u[j] = uj;
    if (tid > j && tid < nn) v[tid] -= Mx[tid + (size_t)j * ld] * uj;
  }
  __syncthreads();
}
// u = L'^-1 v (v is overwritten); reads L' from the upper triangle.
DEVINL void solve_upper(const double* Mx, int ld, int nn, double* v, double* u) {
  const int tid = threadIdx.x;
  for (int j = nn - 1; j >= 0; --j) {
    __syncthreads();
    const double uj = v[j] / Mx[j + (size_t)j * ld];
    if (tid == 0) u[j] = uj;
    if (tid < j) v[tid] -= Mx[tid + (size_t)j * ld] * uj;
  }
  __syncthreads();
}

__global__ __launch_bounds__(QPS_THREADS) void qp_vjp_kernel(QpsParams P) {
  extern __shared__ double smem[];
  const int n = P.n, m = P.m, np = P.np, ldm = P.ldm, k = P.k;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // ---- LDS carve (qps_plan mirrors it) ----
  double* sp = smem;
  double* Ml = nullptr;
  if (P.m_in_lds) { Ml = sp; sp += (size_t)np * ldm; }
  double* XS = sp;  sp += np;   // x
  double* DF = sp;  sp += np;   // column scale of free variable p
  double* RW = sp;  sp += np;   // row scale of working row q
  double* R1 = sp;  sp += np;   // right-hand sides / residuals (scaled, free part)
  double* R2 = sp;  sp += np;   //   (scaled, working rows)
  double* U = sp;   sp += np;
  double* T1 = sp;  sp += np;
  double* T2 = sp;  sp += np;
  double* DW = sp;  sp += np;
  double* DMU = sp; sp += np;
  double* WT = sp;  sp += np;   // w~ (free part, scaled)
  double* MUT = sp; sp += np;   // mu~ (working rows, scaled)
  double* WF = sp;  sp += np;   // w over all n variables (unscaled, 0 on pinned ones)
  double* HXG = sp; sp += np;   // H x + g
  double* XB = sp;  sp += np;   // effective cotangent xbar + fbar (H x + g)
  double* red = sp; sp += 8;
  int* SB = (int*)sp;           // side of variable i's bound in W (-1 lower, +1 upper, 0 free)
  int* IF = SB + np;            // free variables, in order
  int* IW = IF + np;            // working rows, in order
  int* SW = IW + np;            // their sides
  int* cnt = SW + np;           // [0] nF, [1] nW, [2] failed, [3] weak

  for (int b = blockIdx.x; b < P.B; b += gridDim.x) {
    double* ws = P.ws + (size_t)blockIdx.x * P.ws_per_slot;
    double* Aw = ws;                             // np x np, row q = working row (scaled), column p = free variable
    double* Yt = Aw + (size_t)np * np;           // np x np, Yt[i][q] = (L^-1 A~')[i][q]
    double* S = Yt + (size_t)np * np;            // np x ldm
    double* M = P.m_in_lds ? Ml : S + (size_t)np * ldm;
    int* rowpos = (int*)(S + (size_t)np * ldm + (P.m_in_lds ? 0 : (size_t)np * ldm));   // m ints: position of row r in W, or -1
    const size_t oH = P.shared_HA ? 0 : (size_t)b * n * n, oA = P.shared_HA ? 0 : (size_t)b * m * n;
    const double* H = P.H + oH; const double* A = P.A ? P.A + oA : nullptr;
    const double* g = P.g + (size_t)b * n;
    const double* lb = P.lb + (size_t)b * n; const double* ub = P.ub + (size_t)b * n;
    const double* lbA = m ? P.lbA + (size_t)b * m : nullptr; const double* ubA = m ? P.ubA + (size_t)b * m : nullptr;
    const double* lam = P.lam + (size_t)b * (n + m);
    const int ef = P.exitflag[b];
    const int pol = P.polished ? P.polished[b] : 0;
    const double ib = P.inf_bound;
    int status = QPS_FWD;
    if (ef == 0) {
      // ---- working set (the rule of the solver's refinement) ----
      for (int i = tid; i < np; i += QPS_THREADS) {
        const double xi = i < n ? P.x[(size_t)b * n + i] : 0.0;
        XS[i] = xi;
        int s = 0;
        if (i < n) {
          const double l = lb[i], u = ub[i], li = lam[i];
          if (l > -ib && li > 0 && li > fabs(xi - l)) s = -1;
          else if (u < ib && li < 0 && -li > fabs(u - xi)) s = 1;
        }
        SB[i] = s;
      }
      __syncthreads();
      double lmax = 0.0;
      for (int i = tid; i < n + m; i += QPS_THREADS) lmax = fmax(lmax, fabs(lam[i]));
      for (int r = tid; r < m; r += QPS_THREADS) {
        double v = 0.0;
        for (int j = 0; j < n; ++j) v += A[r + (size_t)j * m] * XS[j];
        const double l = lbA[r], u = ubA[r], lr = lam[n + r];
        int s = 0;
        if (l > -ib && lr > 0 && lr > fabs(v - l)) s = -1;
        else if (u < ib && lr < 0 && -lr > fabs(u - v)) s = 1;
        rowpos[r] = s;
      }
      lmax = block_max(lmax, red);
      // compaction in index order (wave 0, ballots): free variables, then working rows
      if (wave == 0) {
        int c = 0;
        for (int base = 0; base < n; base += 64) {
          const int i = base + lane;
          const bool f = i < n && SB[i] == 0;
          const unsigned long long msk = __ballot(f);
          if (f) IF[c + __popcll(msk & ((1ull << lane) - 1ull))] = i;
          c += __popcll(msk);
        }
        int w = 0;
        for (int base = 0; base < m; base += 64) {
          const int r = base + lane;
          const int s = r < m ? rowpos[r] : 0;
          const unsigned long long msk = __ballot(s != 0);
          const int pos = w + __popcll(msk & ((1ull << lane) - 1ull));
          if (s != 0 && pos < np) { IW[pos] = r; SW[pos] = s; }
          if (r < m) rowpos[r] = s != 0 ? pos : -1;
          w += __popcll(msk);
        }
        if (lane == 0) { cnt[0] = c; cnt[1] = w; cnt[2] = w > c ? 1 : 0; }
      }
      __syncthreads();
      const int nF = cnt[0], nW = cnt[1];
      bool ok = cnt[2] == 0;
      // weakly active: a working-set multiplier at or below tol (1 + |lambda|_inf)
      int weak = 0;
      const double wt = P.tol * (1.0 + lmax);
      for (int i = tid; i < n; i += QPS_THREADS) weak |= SB[i] != 0 && fabs(lam[i]) <= wt;
      if (ok) for (int q = tid; q < nW; q += QPS_THREADS) weak |= fabs(lam[n + IW[q]]) <= wt;
      weak = block_max((double)weak, red) > 0.0;
      const int nFp = rup(nF, 16), nWp = rup(nW, 16);
      if (ok) {
        // ---- scaling: unit diagonal of H~ (columns without curvature: unit max over the working rows), unit max-norm rows of A~ ----
        for (int p = tid; p < nF; p += QPS_THREADS) {
          const int i = IF[p];
          const double h = H[i + (size_t)i * n];
          double d;
          if (h > 0.0) d = 1.0 / sqrt(h);
          else {
            double a = 0.0;
            for (int q = 0; q < nW; ++q) a = fmax(a, fabs(A[IW[q] + (size_t)i * m]));
            d = a > 0.0 ? 1.0 / a : 1.0;
          }
          DF[p] = d;
        }
        __syncthreads();
        const int Kw = rup(nW, 4);
        for (size_t e = tid; e < (size_t)Kw * np; e += QPS_THREADS) Aw[e] = 0.0;
        __syncthreads();
        for (int q = wave; q < nW; q += 4) {   // one wave per row: max-norm, then the scaled row
          const int r = IW[q];
          double a = 0.0;
          for (int p = lane; p < nF; p += 64) a = fmax(a, fabs(A[r + (size_t)IF[p] * m] * DF[p]));
          for (int o = 32; o > 0; o >>= 1) a = fmax(a, __shfl_xor(a, o));
          const double rs = a > 0.0 ? 1.0 / a : 1.0;
          if (lane == 0) RW[q] = rs;
          for (int p = lane; p < nF; p += 64) Aw[(size_t)q * np + p] = rs * A[r + (size_t)IF[p] * m] * DF[p];
        }
        __syncthreads();
        // ---- M = H~_FF + rho A~'A~ (MFMA), Cholesky ----
        syrk_lower(Aw, np, Kw, nFp, M, ldm, RHO, [&](int r, int c) -> double {
          if (r < nF && c < nF) return DF[r] * H[IF[r] + (size_t)IF[c] * n] * DF[c];
          return r == c ? 1.0 : 0.0;
        });
        ok = cholesky(M, ldm, nF);
      }
      if (ok && nW > 0) {
        // ---- Y = L^-1 A~' (one column per thread), S = Y'Y (MFMA), Cholesky ----
        const int KF = rup(nF, 4);
        for (size_t e = tid; e < (size_t)KF * np; e += QPS_THREADS) Yt[e] = 0.0;
        __syncthreads();
        if (tid < nW) {
          for (int i = 0; i < nF; ++i) {
            double s = Aw[(size_t)tid * np + i];
            for (int j = 0; j < i; ++j) s -= M[i + (size_t)j * ldm] * Yt[(size_t)j * np + tid];
            Yt[(size_t)i * np + tid] = s / M[i + (size_t)i * ldm];
          }
        }
        __syncthreads();
        syrk_lower(Yt, np, KF, nWp, S, ldm, 1.0, [&](int r, int c) -> double { return (r >= nW && r == c) ? 1.0 : 0.0; });
        ok = cholesky(S, ldm, nW);
      }
      // H x + g (for the fval cotangent)
      if (ok && P.fbar)
        for (int i = tid; i < n; i += QPS_THREADS) {
          double s = g[i];
          for (int j = 0; j < n; ++j) s += H[i + (size_t)j * n] * XS[j];
          HXG[i] = s;
        }
      __syncthreads();
      double worst = 0.0;
      for (int c = 0; c < k && ok; ++c) {
        const double fb = P.fbar ? P.fbar[(size_t)b * k + c] : 0.0;
        const double* xb = P.xbar + ((size_t)b * k + c) * n;
        for (int i = tid; i < n; i += QPS_THREADS) XB[i] = xb[i] + (fb != 0.0 ? fb * HXG[i] : 0.0);
        __syncthreads();
        for (int p = tid; p < np; p += QPS_THREADS) { R1[p] = p < nF ? DF[p] * XB[IF[p]] : 0.0; R2[p] = 0.0; WT[p] = 0.0; MUT[p] = 0.0; }
        double rnorm = 0.0;
        for (int p = tid; p < nF; p += QPS_THREADS) rnorm = fmax(rnorm, fabs(DF[p] * XB[IF[p]]));
        rnorm = block_max(rnorm, red);
        double err = INFINITY, prev = INFINITY;
        for (int it = 0; it < QPS_MAX_REFINE; ++it) {
          // (dw, dmu) solves [H~ A~'; A~ 0] (dw, dmu) = (R1, R2):  r' = R1 + rho A~'R2,  u = L^-1 r',  S dmu = Y'u - R2,  dw = L'^-1 (u - Y dmu)
          for (int p = tid; p < nF; p += QPS_THREADS) {
            double s = R1[p];
            for (int q = 0; q < nW; ++q) s += RHO * Aw[(size_t)q * np + p] * R2[q];
            R1[p] = s;
          }
          solve_lower(M, ldm, nF, R1, U);
          if (nW > 0) {
            if (tid < nW) {
              double s = -R2[tid];
              for (int i = 0; i < nF; ++i) s += Yt[(size_t)i * np + tid] * U[i];
              T1[tid] = s;
            }
            solve_lower(S, ldm, nW, T1, T2);
            solve_upper(S, ldm, nW, T2, DMU);
            if (tid < nF) {
              double s = U[tid];
              for (int q = 0; q < nW; ++q) s -= Yt[(size_t)tid * np + q] * DMU[q];
              U[tid] = s;
            }
            __syncthreads();
          }
          solve_upper(M, ldm, nF, U, DW);
          for (int p = tid; p < nF; p += QPS_THREADS) WT[p] += DW[p];
          for (int q = tid; q < nW; q += QPS_THREADS) MUT[q] += DMU[q];
          __syncthreads();
          // residual of the scaled adjoint system at (w~, mu~)
          for (int p = tid; p < nF; p += QPS_THREADS) {
            double s = DF[p] * XB[IF[p]];
            double hw = 0.0;
            for (int q = 0; q < nF; ++q) hw += H[IF[p] + (size_t)IF[q] * n] * (DF[q] * WT[q]);
            s -= DF[p] * hw;
            for (int q = 0; q < nW; ++q) s -= Aw[(size_t)q * np + p] * MUT[q];
            R1[p] = s;
          }
          for (int q = tid; q < nW; q += QPS_THREADS) {
            double s = 0.0;
            for (int p = 0; p < nF; ++p) s -= Aw[(size_t)q * np + p] * WT[p];
            R2[q] = s;
          }
          double e = 0.0, sc = rnorm;
          for (int p = tid; p < nF; p += QPS_THREADS) { e = fmax(e, fabs(R1[p])); sc = fmax(sc, fabs(WT[p])); }
          for (int q = tid; q < nW; q += QPS_THREADS) { e = fmax(e, fabs(R2[q])); sc = fmax(sc, fabs(MUT[q])); }
          e = block_max(e, red); sc = block_max(sc, red);
          err = sc > 0.0 ? e / sc : 0.0;
          // refine until the residual stagnates (or reaches rounding level): the last passes cost little and leave no avoidable error
          if (err <= 1e-16 || err > 0.5 * prev) break;
          prev = err;
        }
        if (!(err <= 1e-12)) { ok = false; break; }
        worst = fmax(worst, err);
        // ---- outputs of column c ----
        for (int i = tid; i < n; i += QPS_THREADS) WF[i] = 0.0;
        __syncthreads();
        for (int p = tid; p < nF; p += QPS_THREADS) WF[IF[p]] = DF[p] * WT[p];
        __syncthreads();
        const size_t on = ((size_t)b * k + c) * n, om = ((size_t)b * k + c) * m;
        for (int i = tid; i < n; i += QPS_THREADS) {
          P.gbar[on + i] = -WF[i] + fb * XS[i];
          double mu = 0.0;
          if (SB[i] != 0) {   // pinned: multiplier from the stationarity row i
            mu = XB[i];
            for (int j = 0; j < n; ++j) mu -= H[i + (size_t)j * n] * WF[j];
            for (int q = 0; q < nW; ++q) mu -= A[IW[q] + (size_t)i * m] * (RW[q] * MUT[q]);
          }
          if (P.lbbar) P.lbbar[on + i] = SB[i] < 0 ? mu : 0.0;
          if (P.ubbar) P.ubbar[on + i] = SB[i] > 0 ? mu : 0.0;
        }
        for (int r = tid; r < m; r += QPS_THREADS) {
          const int q = rowpos[r];
          const double mu = q >= 0 ? RW[q] * MUT[q] : 0.0;
          if (P.lbAbar) P.lbAbar[om + r] = (q >= 0 && SW[q] < 0) ? mu : 0.0;
          if (P.ubAbar) P.ubAbar[om + r] = (q >= 0 && SW[q] > 0) ? mu : 0.0;
        }
        if (P.Hbar) {
          double* Hb = P.Hbar + ((size_t)b * k + c) * n * n;
          for (size_t e = tid; e < (size_t)n * n; e += QPS_THREADS) {
            const int i = (int)(e % n), j = (int)(e / n);
            Hb[e] = -0.5 * (WF[i] * XS[j] + XS[i] * WF[j]) + 0.5 * fb * XS[i] * XS[j];
          }
        }
        if (P.Abar) {
          double* Ab = P.Abar + ((size_t)b * k + c) * m * n;
          for (size_t e = tid; e < (size_t)m * n; e += QPS_THREADS) {
            const int r = (int)(e % m), j = (int)(e / m);
            const int q = rowpos[r];
            Ab[e] = q >= 0 ? lam[n + r] * WF[j] - RW[q] * MUT[q] * XS[j] : 0.0;
          }
        }
        __syncthreads();
      }
      status = !ok ? QPS_SINGULAR : (pol <= 0 ? QPS_IPM : (weak ? QPS_WEAK : QPS_OK));
    }
    if (status < 0) {   // zeros
      for (int c = 0; c < k; ++c) {
        const size_t on = ((size_t)b * k + c) * n, om = ((size_t)b * k + c) * m;
        for (int i = tid; i < n; i += QPS_THREADS) {
          P.gbar[on + i] = 0.0;
          if (P.lbbar) P.lbbar[on + i] = 0.0;
          if (P.ubbar) P.ubbar[on + i] = 0.0;
        }
        for (int r = tid; r < m; r += QPS_THREADS) {
          if (P.lbAbar) P.lbAbar[om + r] = 0.0;
          if (P.ubAbar) P.ubAbar[om + r] = 0.0;
        }
        if (P.Hbar) for (size_t e = tid; e < (size_t)n * n; e += QPS_THREADS) P.Hbar[((size_t)b * k + c) * n * n + e] = 0.0;
        if (P.Abar) for (size_t e = tid; e < (size_t)m * n; e += QPS_THREADS) P.Abar[((size_t)b * k + c) * m * n + e] = 0.0;
      }
    }
    if (tid == 0) P.status[b] = status;
    __syncthreads();
  }
}
}  // namespace

size_t qps_plan(QpsParams* P) {
  P->np = (P->n + 15) / 16 * 16;
  P->ldm = P->np + 1;
  const size_t mat = (size_t)P->np * P->ldm * sizeof(double);
  const size_t vec = ((size_t)15 * P->np + 8 + 2 * (size_t)P->np) * sizeof(double) + 16 * sizeof(int);
  P->m_in_lds = P->np <= 128 ? 1 : 0;
  P->lds_bytes = vec + (P->m_in_lds ? mat : 0);
  P->slots = P->B < QPS_MAX_SLOTS ? P->B : QPS_MAX_SLOTS;
  const size_t per = (size_t)2 * P->np * P->np + (size_t)(P->m_in_lds ? 1 : 2) * P->np * P->ldm + ((size_t)P->m + 1) / 2 + 8;
  P->ws_per_slot = (per + 31) / 32 * 32;
  return (size_t)P->slots * P->ws_per_slot * sizeof(double);
}

hipError_t qps_launch(const QpsParams& P, hipStream_t st) {
  if (P.B == 0) return hipSuccess;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&qp_vjp_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.lds_bytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(qp_vjp_kernel, dim3(P.slots), dim3(QPS_THREADS), P.lds_bytes, st, P);
  return hipGetLastError();
}
