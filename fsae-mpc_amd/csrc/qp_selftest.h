// qp_selftest.h -- device self tests of the QP kernels' building blocks (main unit of qp_solver.hip only): fp64 MFMA lane maps, the
// lane reductions of qp_lane.h, the forms of diag_factor, the start-up pass.  Kernels and their host entry points.
#pragma once
#include <stdlib.h>
#include <stdio.h>
#include "qp_solve_kernel.h"

namespace {

// ---------------------------------------------------------------------------------------------
// MFMA layout self test
// ---------------------------------------------------------------------------------------------
__global__ void mfma_selftest_kernel(const double* Am, const double* Bm, double* Cm) {
  // Am: 16x4 row-major (A[i][k]), Bm: 4x16 row-major (B[k][j]), Cm: 16x16 row-major out
  const int lane = threadIdx.x;
  const double a = Am[(lane & 15) * 4 + (lane >> 4)];
  const double bb = Bm[(lane >> 4) * 16 + (lane & 15)];
  v4d c = {0, 0, 0, 0};
  c = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bb, c, 0, 0, 0);
#pragma unroll
  for (int p = 0; p < 4; ++p) Cm[((lane >> 4) + 4 * p) * 16 + (lane & 15)] = c[p];
}

// ---------------------------------------------------------------------------------------------
// Lane-reduction self test: one wave, all lanes active.  Every reduction (single, batched, 16-lane row / four rows / whole wave) is
// compared bit for bit (NaN = NaN) with the zero-filling lane moves and with a plain tree through LDS that pairs the same lanes
// in the same order: lane^1, lane^2, lane <-> 7-lane within 8, lane <-> 15-lane within 16, rows 0<->1 and 2<->3, halves.
// ---------------------------------------------------------------------------------------------
DEVINL bool same_bits(double a, double b) { return __double_as_longlong(a) == __double_as_longlong(b) || (a != a && b != b); }
template <class OP> DEVINL double lds_grp16(double* sh, int lane, double v) {
  const int src[4] = {lane ^ 1, lane ^ 2, (lane & ~7) | (7 - (lane & 7)), (lane & ~15) | (15 - (lane & 15))};
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    sh[lane] = v; __syncthreads();
    const double o = sh[src[s]]; __syncthreads();
    v = OP::f(v, o);
  }
  return v;
}
template <class OP> DEVINL double lds_q(double* sh, int lane, double v) {   // (row0,row1) -> row0 op row1 on both, as the lane swaps give it
#pragma unroll
  for (int bit = 16; bit <= 32; bit <<= 1) {
    sh[lane] = v; __syncthreads();
    const double a = sh[lane & ~bit], b = sh[lane | bit]; __syncthreads();
    v = OP::f(a, b);
  }
  return v;
}
DEVINL double q_named(OpSum, double v) { return q_sum(v); }
DEVINL double q_named(OpMax, double v) { return q_max(v); }
DEVINL double q_named(OpMin, double v) { return q_min(v); }
DEVINL double wave_named(OpSum, double v) { return wave_sum(v); }
DEVINL double wave_named(OpMax, double v) { return wave_max(v); }
DEVINL double wave_named(OpMin, double v) { return wave_min(v); }
DEVINL double wave_named_zf(OpSum, double v) { return wave_sum_zf(v); }
DEVINL double wave_named_zf(OpMax, double v) { return wave_max_zf(v); }
DEVINL double wave_named_zf(OpMin, double v) { return wave_min_zf(v); }
DEVINL double grp16_named(OpSum, double v) { return grp16_sum(v); }
DEVINL double grp16_named(OpMax, double v) { return grp16_max(v); }
DEVINL double grp16_named(OpMin, double v) { return grp16_min(v); }
template <int N> DEVINL void grp16_named(OpSum, double (&v)[N]) { grp16_sum(v); }
template <int N> DEVINL void grp16_named(OpMax, double (&v)[N]) { grp16_max(v); }
template <int N> DEVINL void grp16_named(OpMin, double (&v)[N]) { grp16_min(v); }
template <class OP, int N> DEVINL int lane_reduce_batch_bad(const double (&x)[8], const double (&rz)[8], const double (&rl_)[8]) {
  double a[N];
#pragma unroll
  for (int i = 0; i < N; ++i) a[i] = x[i];
  grp16_named(OP{}, a);
  int bad = 0;
#pragma unroll
  for (int i = 0; i < N; ++i) bad += (same_bits(a[i], rz[i]) ? 0 : 1) + (same_bits(a[i], rl_[i]) ? 0 : 1);
  return bad;
}
// returns this lane's number of mismatches; `first` gets a code (100 * test + op) of the first kind of test that failed
template <class OP> DEVINL int lane_reduce_op_bad(int op, double* sh, int lane, const double (&x)[8], int& first) {
  double rz[8], rl_[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    double z[1] = {x[i]};
    grp16_reduce<OP, true>(z);
    rz[i] = z[0];
    rl_[i] = lds_grp16<OP>(sh, lane, x[i]);
  }
  int bad = 0, b;
  auto note = [&](int test, int nb) { if (nb && first < 0) first = 100 * test + op; bad += nb; };
  { const double g = grp16_named(OP{}, x[0]); note(1, (same_bits(g, rz[0]) ? 0 : 1) + (same_bits(g, rl_[0]) ? 0 : 1)); }
  b = lane_reduce_batch_bad<OP, 2>(x, rz, rl_); note(2, b);
  b = lane_reduce_batch_bad<OP, 4>(x, rz, rl_); note(4, b);
  b = lane_reduce_batch_bad<OP, 8>(x, rz, rl_); note(8, b);
  { const double g = q_named(OP{}, x[1]); note(16, same_bits(g, lds_q<OP>(sh, lane, x[1])) ? 0 : 1); }
  {
    const double g = wave_named(OP{}, x[2]), z = wave_named_zf(OP{}, x[2]), l = lds_q<OP>(sh, lane, rl_[2]);
    note(64, (same_bits(g, z) ? 0 : 1) + (same_bits(g, l) ? 0 : 1));
  }
  return bad;
}
__global__ __launch_bounds__(64) void lane_reduce_selftest_kernel(const double* __restrict__ in, int rounds, int* __restrict__ out) {
  __shared__ double sh[64];
  const int lane = threadIdx.x;
  int bad = 0, first = -1, first_round = -1;
  for (int r = 0; r < rounds; ++r) {   // (uniform trip count: every lane stays active)
    double x[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = in[((size_t)r * 8 + i) * 64 + lane];
    const int before = bad;
    bad += lane_reduce_op_bad<OpSum>(0, sh, lane, x, first);
    bad += lane_reduce_op_bad<OpMax>(1, sh, lane, x, first);
    bad += lane_reduce_op_bad<OpMin>(2, sh, lane, x, first);
    {   // adjacent whole-wave sums as one batch
      double a[4] = {x[4], x[5], x[6], x[7]};
      wave_sum(a);
      int nb = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) nb += same_bits(a[i], wave_sum_zf(x[4 + i])) ? 0 : 1;
      if (nb && first < 0) first = 100 * 65;
      bad += nb;
    }
    if (bad != before && first_round < 0) first_round = r;
  }
  if (bad) {
    if (atomicAdd(&out[0], bad) == 0) { out[1] = first; out[2] = first_round; out[3] = lane; }
  }
}

// ---------------------------------------------------------------------------------------------
// diag_factor self test: one wave, all lanes active.  Every tile goes through the former form (FORM 0) and through the two newer
// ones; the diagonal tile, both companions and the flag must agree bit for bit (also where they are NaN).
// in: per tile 512 doubles, the diagonal tile and the right-hand-side tile, row-major 16 x 16.  out: {mismatches, first tile, form, lane}.
// ---------------------------------------------------------------------------------------------
template <int FORM> DEVINL int diag_factor_bad_vs_old(const Ctx& k, const v4d& U0, const v4d& R0, double floor_abs, const v4d& Uo, const v4d& Yo, const v4d& Ro, int bo) {
  v4d U = U0, R = R0, Y;
#pragma unroll
  for (int p = 0; p < 4; ++p) Y[p] = (k.q + 4 * p == k.c) ? 1.0 : 0.0;
  const int b = diag_factor<FORM>(k, U, Y, R, floor_abs);
  int bad = (b != bo) ? 1 : 0;
#pragma unroll
  for (int p = 0; p < 4; ++p)
    bad += (__double_as_longlong(U[p]) != __double_as_longlong(Uo[p])) + (__double_as_longlong(Y[p]) != __double_as_longlong(Yo[p])) +
           (__double_as_longlong(R[p]) != __double_as_longlong(Ro[p]));
  return bad;
}
__global__ __launch_bounds__(64) void diag_factor_selftest_kernel(const double* __restrict__ in, int ntiles, double floor_abs, int* __restrict__ out) {
  Ctx k = {};
  k.lane = threadIdx.x; k.c = k.lane & 15; k.q = k.lane >> 4;
  int bad = 0, first = -1, form = 0;
  for (int t = 0; t < ntiles; ++t) {   // (uniform trip count: every lane stays active)
    v4d U0, R0, Uo, Ro, Yo;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      U0[p] = in[(size_t)t * 512 + (k.q + 4 * p) * 16 + k.c];
      R0[p] = in[(size_t)t * 512 + 256 + (k.q + 4 * p) * 16 + k.c];
      Yo[p] = (k.q + 4 * p == k.c) ? 1.0 : 0.0;
    }
    Uo = U0; Ro = R0;
    const int bo = diag_factor<0>(k, Uo, Yo, Ro, floor_abs);
    const int b1 = diag_factor_bad_vs_old<1>(k, U0, R0, floor_abs, Uo, Yo, Ro, bo);
    const int b2 = diag_factor_bad_vs_old<2>(k, U0, R0, floor_abs, Uo, Yo, Ro, bo);
    if ((b1 | b2) && first < 0) { first = t; form = b1 ? 1 : 2; }
    bad += b1 + b2;
  }
  if (bad) {
    if (atomicAdd(&out[0], bad) == 0) { out[1] = first; out[2] = form; out[3] = k.lane; }
  }
}

// ---------------------------------------------------------------------------------------------
// Initial-point self test: one wave on one QP that qp_prep_kernel has prepared.  aV = A~ x and P3 = A~'w of the initial multipliers
// are computed the former way (pass_Av<.., 1, 0>, then pass_Atw) and by the start-up pass of the solve kernel (pass_Av<.., 1, -1>);
// both vectors must agree bit for bit (also where they are NaN).  out: {mismatches, first kind (0: aV, 1: P3), index, lane, nonzeros}.
// ---------------------------------------------------------------------------------------------
template <int T, int NB> __global__ __launch_bounds__(64) void initial_point_selftest_kernel(QpParams P, int* __restrict__ out) {
  extern __shared__ double lds[];
  Ctx k;
  (void)ctx_setup<T>(k, P, 0, lds);
  const QpSolveLds L = qp_solve_lds(T, NB, P.d.np);
  k.ring = lds + L.vecs + L.border + L.tiles;
  k.cof = k.ring + L.ring;
  const int lane = k.lane, J = k.J, JT = k.JT;
  double* Xv = vecp(k, V_X); double* P3o = vecp(k, V_P1); double* P3n = vecp(k, V_P3);
  double* W3 = rowp(k, R_W3); double* Vo = rowp(k, R_VA); double* Vn = rowp(k, R_V);
  const double* Lb = rowp(k, R_L); const double* Ub = rowp(k, R_U);
  Stream<T> st;
  st.open(k);
  for (int js = 0; js < JT; ++js) {   // the weights as the solve kernel sets them: by the finiteness of the bounds; x inside its bounds
    const int ix = js * 64 + lane;
    const bool valid = row_valid(k, js);
    const double l = Lb[ix], u = Ub[ix];
    W3[ix] = (valid && js < J) ? ((l > -INFINITY ? 100.0 : 0.0) - (u < INFINITY ? 100.0 : 0.0)) : 0.0;
    if (js >= J) {
      const int i = (js - J) * 64 + lane;
      if (i < k.np) {
        double xi = i < k.n ? 0.375 * ((i * 7) % 5 - 2) + 0.01 * i : 0.0;
        if (valid) { if (l > -INFINITY && xi < l) xi = l; if (u < INFINITY && xi > u) xi = u; }
        Xv[i] = xi;
      }
    }
  }
  WAVE_SYNC();
  const double* vin[1] = {Xv};
  { double* rout[1] = {Vo}; pass_Av<T, NB, 1, 0>(k, st, vin, rout, nullptr); }
  pass_Atw<T, NB>(k, W3, P3o);
  WAVE_SYNC();
  { double* rout[1] = {Vn}; pass_Av<T, NB, 1, -1>(k, st, vin, rout, P3n); }
  WAVE_SYNC();
  st.close();
  int bad = 0, kind = -1, at = -1, nz = 0;
  for (int js = 0; js < J; ++js) {
    const int ix = js * 64 + lane;
    if (!same_bits(Vo[ix], Vn[ix])) { if (!bad) { kind = 0; at = ix; } ++bad; }
    nz += Vo[ix] != 0.0;
  }
  for (int i = lane; i < k.nc + NB; i += 64) {
    if (!same_bits(P3o[i], P3n[i])) { if (!bad) { kind = 1; at = i; } ++bad; }
    nz += P3o[i] != 0.0;
  }
  if (nz) atomicAdd(&out[4], nz);
  if (bad) {
    if (atomicAdd(&out[0], bad) == 0) { out[1] = kind; out[2] = at; out[3] = lane; }
  }
}

}  // namespace

int qp_selftest_mfma(char* msg, int msglen) {
  double hA[64], hB[64], hC[256], ref[256];
  for (int i = 0; i < 16; ++i) for (int kk = 0; kk < 4; ++kk) hA[i * 4 + kk] = (double)(1 + i * 7 + kk * 3);   // asymmetric integers
  for (int kk = 0; kk < 4; ++kk) for (int j = 0; j < 16; ++j) hB[kk * 16 + j] = (double)(2 + kk * 11 - j * 5);
  for (int i = 0; i < 16; ++i) for (int j = 0; j < 16; ++j) {
    double s = 0; for (int kk = 0; kk < 4; ++kk) s += hA[i * 4 + kk] * hB[kk * 16 + j];
    ref[i * 16 + j] = s;
  }
  double *dA = 0, *dB = 0, *dC = 0;
  if (hipMalloc(&dA, sizeof(hA)) != hipSuccess || hipMalloc(&dB, sizeof(hB)) != hipSuccess || hipMalloc(&dC, sizeof(hC)) != hipSuccess) return -1;
  (void)hipMemcpy(dA, hA, sizeof(hA), hipMemcpyHostToDevice);
  (void)hipMemcpy(dB, hB, sizeof(hB), hipMemcpyHostToDevice);
  (void)hipMemset(dC, 0, sizeof(hC));
  hipLaunchKernelGGL(mfma_selftest_kernel, dim3(1), dim3(64), 0, 0, dA, dB, dC);
  hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) { snprintf(msg, msglen, "selftest launch: %s", hipGetErrorString(e)); (void)hipFree(dA); (void)hipFree(dB); (void)hipFree(dC); return -1; }
  (void)hipMemcpy(hC, dC, sizeof(hC), hipMemcpyDeviceToHost);
  (void)hipFree(dA); (void)hipFree(dB); (void)hipFree(dC);
  int bad = 0;
  for (int i = 0; i < 256; ++i) if (hC[i] != ref[i]) { if (!bad) snprintf(msg, msglen, "mfma layout mismatch at (%d,%d): got %g want %g", i / 16, i % 16, hC[i], ref[i]); ++bad; }
  return bad;
}

int qp_selftest_lane_reduce(char* msg, int msglen) {
  const int rounds = 256, nval = rounds * 8 * 64;
  double* h = (double*)malloc(sizeof(double) * nval);
  if (!h) return -1;
  unsigned long long st = 0x9E3779B97F4A7C15ull;   // fixed seed
  auto rnd = [&]() { st = st * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(st >> 33); };
  for (int i = 0; i < nval; ++i) {   // magnitudes 1e-300 .. 1e300, both signs
    const double e = -300.0 + 600.0 * (rnd() / 2147483648.0), m = 1.0 + 9.0 * (rnd() / 2147483648.0);
    h[i] = ((rnd() & 1) ? -1.0 : 1.0) * m * pow(10.0, e);
  }
  const double special[8] = {0.0, -0.0, 4.9406564584124654e-324, -2.2250738585072009e-308 / 3.0, INFINITY, -INFINITY, NAN, -NAN};
  for (int g = 0; g < rounds * 8; ++g) {   // three of four 64-lane vectors get one special value in a single lane
    const unsigned u = rnd();
    if ((u & 3) != 0) h[(size_t)g * 64 + ((u >> 2) & 63)] = special[(u >> 8) & 7];
    if ((u & 0x30000) == 0x30000) h[(size_t)g * 64 + ((u >> 18) & 63)] = special[(u >> 24) & 7];   // sometimes a second one
  }
  double* d = 0; int* dout = 0; int hout[4] = {0, 0, 0, 0};
  if (hipMalloc(&d, sizeof(double) * nval) != hipSuccess || hipMalloc(&dout, sizeof(hout)) != hipSuccess) { free(h); if (d) (void)hipFree(d); return -1; }
  (void)hipMemcpy(d, h, sizeof(double) * nval, hipMemcpyHostToDevice);
  (void)hipMemset(dout, 0, sizeof(hout));
  free(h);
  hipLaunchKernelGGL(lane_reduce_selftest_kernel, dim3(1), dim3(64), 0, 0, d, rounds, dout);
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(hout, dout, sizeof(hout), hipMemcpyDeviceToHost);
  (void)hipFree(d); (void)hipFree(dout);
  if (e != hipSuccess) { snprintf(msg, msglen, "lane-reduce selftest: %s", hipGetErrorString(e)); return -1; }
  if (hout[0]) snprintf(msg, msglen, "lane reductions: %d mismatches, first: test %d (1/2/4/8: grp16 single / batched, 16: q, 64: wave, 65: wave_sum batch) op %d (sum/max/min) round %d lane %d",
                        hout[0], hout[1] / 100, hout[1] % 100, hout[2], hout[3]);
  return hout[0];
}

int qp_selftest_diag_factor(char* msg, int msglen) {
  // 64 tiles: 61 SPD tiles D = Q diag(s) Q' with condition numbers 1 .. 1e10 (Q: a product of Householder reflections), then a tile
  // with a pivot under the floor, one with a NaN and one with +Inf; every tile with a full right-hand-side tile
  const int ntiles = 64;
  const double floor_abs = 1e-9;
  double* h = (double*)malloc(sizeof(double) * ntiles * 512);
  if (!h) return -1;
  unsigned long long st = 0xD1B54A32D192ED03ull;   // fixed seed
  auto rnd = [&]() { st = st * 6364136223846793005ull + 1442695040888963407ull; return ((unsigned)(st >> 33)) / 2147483648.0; };
  for (int t = 0; t < ntiles; ++t) {
    double* D = h + (size_t)t * 512; double* R = D + 256;
    double Q[16][16], sv[16];
    for (int i = 0; i < 16; ++i) for (int j = 0; j < 16; ++j) Q[i][j] = i == j ? 1.0 : 0.0;
    for (int r = 0; r < 3; ++r) {   // Q <- Q (I - 2 v v' / v'v)
      double v[16], vv = 0;
      for (int i = 0; i < 16; ++i) { v[i] = 2.0 * rnd() - 1.0; vv += v[i] * v[i]; }
      for (int i = 0; i < 16; ++i) {
        double qv = 0;
        for (int j = 0; j < 16; ++j) qv += Q[i][j] * v[j];
        for (int j = 0; j < 16; ++j) Q[i][j] -= 2.0 * qv * v[j] / vv;
      }
    }
    const double lc = 10.0 * (t < 61 ? t / 60.0 : 0.3);   // log10 of the condition number
    for (int i = 0; i < 16; ++i) sv[i] = pow(10.0, -lc * i / 15.0);
    for (int i = 0; i < 16; ++i) for (int j = 0; j < 16; ++j) {
      double a = 0;
      for (int l = 0; l < 16; ++l) a += Q[i][l] * sv[l] * Q[j][l];
      D[i * 16 + j] = a;
    }
    for (int i = 0; i < 16; ++i) for (int j = 0; j < i; ++j) D[i * 16 + j] = D[j * 16 + i];   // exactly symmetric
    for (int i = 0; i < 256; ++i) R[i] = 20.0 * rnd() - 10.0;
    if (t == 61) for (int j = 0; j < 16; ++j) { D[6 * 16 + j] *= 1e-6; D[j * 16 + 6] *= 1e-6; }   // pivot 6 falls under the floor
    if (t == 62) { D[5 * 16 + 9] = NAN; D[9 * 16 + 5] = NAN; }
    if (t == 63) D[10 * 16 + 10] = INFINITY;
  }
  double* d = 0; int* dout = 0; int hout[4] = {0, 0, 0, 0};
  if (hipMalloc(&d, sizeof(double) * ntiles * 512) != hipSuccess || hipMalloc(&dout, sizeof(hout)) != hipSuccess) { free(h); if (d) (void)hipFree(d); return -1; }
  (void)hipMemcpy(d, h, sizeof(double) * ntiles * 512, hipMemcpyHostToDevice);
  (void)hipMemset(dout, 0, sizeof(hout));
  free(h);
  hipLaunchKernelGGL(diag_factor_selftest_kernel, dim3(1), dim3(64), 0, 0, d, ntiles, floor_abs, dout);
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(hout, dout, sizeof(hout), hipMemcpyDeviceToHost);
  (void)hipFree(d); (void)hipFree(dout);
  if (e != hipSuccess) { snprintf(msg, msglen, "diag_factor selftest: %s", hipGetErrorString(e)); return -1; }
  if (hout[0]) snprintf(msg, msglen, "diag_factor forms: %d mismatches with the former form, first: tile %d form %d lane %d", hout[0], hout[1], hout[2], hout[3]);
  return hout[0];
}

// One shape of the initial-point self test: a QP with staircase sparsity (row r reaches the core columns up to its own stage, so the
// tile count of the trips varies; the border columns are dense), infinite, one-sided, two-sided and equality bounds.
template <int T, int NB> static hipError_t initial_point_launch(const QpParams& P, int* dout) {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&initial_point_selftest_kernel<T, NB>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.d.lds_solve);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((initial_point_selftest_kernel<T, NB>), dim3(1), dim3(64), P.d.lds_solve, 0, P, dout);
  return hipGetLastError();
}
static int initial_point_shape(int nV, int nC, char* msg, int msglen) {
  QpDims d;
  qp_make_dims(nV, nC, &d);
  const int nb = d.nb, ncu = nV - nb;   // the caller's core columns
  const double inf = 1e20;
  const size_t nH = (size_t)nV * nV, nA = (size_t)nC * nV, nin = nH + nA + 3 * (size_t)nV + 2 * (size_t)nC;
  double* h = (double*)calloc(nin, sizeof(double));
  if (!h) return -1;
  double *H = h, *A = H + nH, *g = A + nA, *lb = g + nV, *ub = lb + nV, *lbA = ub + nV, *ubA = lbA + nC;
  unsigned long long st = 0xA0761D6478BD642Full + (unsigned)nV * 1000003u + (unsigned)nC;   // fixed seed per shape
  auto rnd = [&]() { st = st * 6364136223846793005ull + 1442695040888963407ull; return ((unsigned)(st >> 33)) / 2147483648.0; };
  for (int j = 0; j < nV; ++j) {   // column-major, symmetric, diagonally dominant; a slack column without curvature takes the column-max scale
    for (int i = 0; i < j; ++i) if ((i + j) % 3 == 0) { const double v = 0.1 * (rnd() - 0.5); H[(size_t)j * nV + i] = v; H[(size_t)i * nV + j] = v; }
    H[(size_t)j * nV + j] = (nb > 0 && j == nV - 1) ? 0.0 : 1.0 + 3.0 * rnd();
    g[j] = 2.0 * rnd() - 1.0;
  }
  for (int r = 0; r < nC; ++r) {
    const int reach = ncu > 0 ? 1 + (int)(((long long)(r + 1) * ncu) / nC) : 0;   // staircase: the last core column of the row
    for (int j = 0; j < ncu && j < reach; ++j) if ((r + j) % 4 != 1) A[(size_t)j * nC + r] = 4.0 * rnd() - 2.0;
    for (int j = ncu; j < nV; ++j) A[(size_t)j * nC + r] = -1.0 + 0.5 * rnd();
    const double mid = rnd() - 0.5;
    switch (r % 5) {
      case 0: lbA[r] = mid - 1.0; ubA[r] = mid + 1.0; break;
      case 1: lbA[r] = mid; ubA[r] = 1e30; break;       // lower side only
      case 2: lbA[r] = -1e30; ubA[r] = mid; break;      // upper side only
      case 3: lbA[r] = mid; ubA[r] = mid; break;        // equality
      default: lbA[r] = -1e30; ubA[r] = 1e30; break;    // free row
    }
  }
  for (int j = 0; j < nV; ++j) {
    switch (j % 4) {
      case 0: lb[j] = -1.0; ub[j] = 1.0; break;
      case 1: lb[j] = 0.25; ub[j] = 1e30; break;
      case 2: lb[j] = -1e30; ub[j] = -0.125; break;
      default: lb[j] = -1e30; ub[j] = 1e30; break;
    }
  }
  double *din = 0, *ws = 0; int* dout = 0; int hout[5] = {0, 0, 0, 0, 0};
  hipError_t e = hipMalloc(&din, sizeof(double) * nin);
  if (e == hipSuccess) e = hipMalloc(&ws, sizeof(double) * d.ws_per_qp);
  if (e == hipSuccess) e = hipMalloc(&dout, sizeof(hout));
  if (e == hipSuccess) e = hipMemcpy(din, h, sizeof(double) * nin, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(ws, 0, sizeof(double) * d.ws_per_qp);
  if (e == hipSuccess) e = hipMemset(dout, 0, sizeof(hout));
  free(h);
  if (e == hipSuccess) {
    QpParams P = {};
    P.d = d;
    P.H = din; P.A = din + nH; P.g = P.A + nA; P.lb = P.g + nV; P.ub = P.lb + nV; P.lbA = P.ub + nV; P.ubA = P.lbA + nC;
    P.ws = ws; P.inf_bound = inf;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&qp_prep_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)d.lds_prep);
    if (e == hipSuccess) { hipLaunchKernelGGL(qp_prep_kernel, dim3(1), dim3(256), d.lds_prep, 0, P); e = hipGetLastError(); }
    if (e == hipSuccess) {
      if (d.T == 1 && d.NB == 4) e = initial_point_launch<1, 4>(P, dout);
      else if (d.T == 2 && d.NB == 4) e = initial_point_launch<2, 4>(P, dout);
      else if (d.T == 2 && d.NB == 0) e = initial_point_launch<2, 0>(P, dout);
      else if (d.T == 2 && d.NB == 1) e = initial_point_launch<2, 1>(P, dout);
      else if (d.T == 5 && d.NB == 1) e = initial_point_launch<5, 1>(P, dout);
      else { snprintf(msg, msglen, "initial-point selftest: shape (%d, %d) has T = %d, NB = %d, which the self test does not instantiate (FSAEMPC_SLACK_BORDER set?)", nV, nC, d.T, d.NB); e = hipErrorInvalidValue; }
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(hout, dout, sizeof(hout), hipMemcpyDeviceToHost);
  }
  if (din) (void)hipFree(din);
  if (ws) (void)hipFree(ws);
  if (dout) (void)hipFree(dout);
  if (e != hipSuccess) { if (!msg[0]) snprintf(msg, msglen, "initial-point selftest (%d, %d): %s", nV, nC, hipGetErrorString(e)); return -1; }
  if (hout[0]) { snprintf(msg, msglen, "initial point (%d, %d): %d mismatches between the start-up pass and pass_Av + pass_Atw, first: %s index %d lane %d", nV, nC, hout[0], hout[1] ? "P3" : "aV", hout[2], hout[3]); return hout[0]; }
  if (!hout[4]) { snprintf(msg, msglen, "initial point (%d, %d): both ways gave all zeros, nothing was compared", nV, nC); return 1; }
  return 0;
}

int qp_selftest_initial_point(char* msg, int msglen) {
  // (nV, nC): T = 1 with a four-column border and one padded trip; T = 2 with three border columns and padded k-steps in the last trip;
  // no border; a core padded with dummy variables (one slack column); the headline instantiation
  const int shapes[5][2] = {{20, 5}, {35, 70}, {32, 64}, {25, 72}, {81, 240}};
  int bad = 0;
  msg[0] = 0;
  for (int i = 0; i < 5; ++i) {
    const int rc = initial_point_shape(shapes[i][0], shapes[i][1], msg, msglen);
    if (rc < 0) return rc;
    bad += rc;
    if (rc) break;
  }
  return bad;
}
