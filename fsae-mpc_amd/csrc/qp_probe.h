// qp_probe.h -- diagnostic builds only (-DQP_PROBE, main unit of qp_solver.hip): pieces of the solve kernel timed on their own.
// qp_launch runs them instead of the solve for QpParams::dump_stage 7 / 8 (tools/probe_factor.py, tools/probe_syrk.py).
#pragma once
#include "qp_solve_kernel.h"

// Diagnostic build only: pass 1 alone (same code, no surrounding solver state) to measure what the matrix-core loop
// costs when the register allocator has nothing else to keep alive.  out[b] = cycles per pass, out[batch+b] = checksum.
template <int T, int NB> __global__ __launch_bounds__(64) void syrk_probe_kernel(QpParams P, int reps) {
  const int b = blockIdx.x;
  extern __shared__ double lds[];
  Ctx k;
  ctx_setup<T>(k, P, b, lds);
  const QpSolveLds L = qp_solve_lds(T, NB, P.d.np);
  double* MB = lds + L.vecs;
  k.ring = MB + L.border + L.tiles; k.cof = k.ring + L.ring;
  for (int js = 0; js < k.JT; ++js) {
    const int ix = js * 64 + k.lane;
    rowp(k, R_D)[ix] = 1.0; rowp(k, R_W1)[ix] = 0.5; rowp(k, R_W2)[ix] = 0.25; rowp(k, R_W3)[ix] = 2.0;
  }
  __syncthreads();
  v4d acc[Tri<T>::NT];
  acc_init<T>(k, acc);
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  for (int r = 0; r < reps; ++r) {   // a fresh stream per repetition: the cost of one pass from a cold start
    Stream<T> st;
    st.open(k);
    pass_syrk<T, NB>(k, st, acc, vecp(k, V_P1), vecp(k, V_P2), vecp(k, V_P3), MB);
    st.close();
    __syncthreads();
  }
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  double cs = 0;
#pragma unroll
  for (int i = 0; i < Tri<T>::NT; ++i) cs += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
  cs = wave_sum(cs);
  if (k.lane == 0) { P.dump[b] = (double)(t1 - t0) / reps; P.dump[gridDim.x + b] = cs; }
}

// Diagnostic build only: does fp64 VALU work run beside fp64 MFMAs of the same wave?  Three loops of `reps` trips: 16 MFMAs (two on
// each of 8 accumulators); 32 v_fma_f64 (four on each of 8 chains); both, 2 FMAs behind every MFMA.  out[0..2] = cycles per trip of
// each (block 0), out[3] = checksum.  One wave per SIMD when launched with the batch as the grid, as the solver runs.
__global__ __launch_bounds__(64) void overlap_probe_kernel(double* out, int reps) {
  const double x = 1.0 + 1e-9 * threadIdx.x, y = 1e-12 * (threadIdx.x + 1);
  v4d acc[8]; double f[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) { acc[i] = v4d{0.0, 0.0, 0.0, 0.0}; f[i] = 1.0 + i; }
  __builtin_amdgcn_sched_barrier(0);
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  for (int r = 0; r < reps; ++r) {
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i & 7] = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, acc[i & 7], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  for (int r = 0; r < reps; ++r) {
#pragma unroll
    for (int i = 0; i < 32; ++i) f[i & 7] = fma(f[i & 7], x, y);
    __builtin_amdgcn_sched_barrier(0);
  }
  const unsigned long long t2 = __builtin_amdgcn_s_memtime();
  for (int r = 0; r < reps; ++r) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      acc[i & 7] = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, acc[i & 7], 0, 0, 0);
      f[(2 * i) & 7] = fma(f[(2 * i) & 7], x, y); f[(2 * i + 1) & 7] = fma(f[(2 * i + 1) & 7], x, y);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) { __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x002, 2, 0); }
    __builtin_amdgcn_sched_barrier(0);
  }
  const unsigned long long t3 = __builtin_amdgcn_s_memtime();
  double cs = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) cs += acc[i][0] + acc[i][3] + f[i];
  cs = wave_sum(cs);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    out[0] = (double)(t1 - t0) / reps; out[1] = (double)(t2 - t1) / reps; out[2] = (double)(t3 - t2) / reps; out[3] = cs;
  }
}

// Diagnostic build only: the register Cholesky alone.  out[b][0..5] = cycles of: whole reg_factor, T diag_factor calls,
// T LDS round trips (tile_store + tile_load_t), forward+backward solve of one right-hand side (vec_forward + vec_backward: the
// solves that ship).
template <int T> __global__ __launch_bounds__(64) void factor_probe_kernel(QpParams P, int reps) {
  const int b = blockIdx.x;
  extern __shared__ double lds[];
  Ctx k;
  ctx_setup<T>(k, P, b, lds);
  const QpSolveLds L = qp_solve_lds(T, 1, P.d.np);
  double* YL = lds + L.vecs + L.border;
  k.ring = YL + L.tiles; k.cof = k.ring + L.ring;
  double* RV = vecp(k, V_R1);   // the right-hand side, then the solution
  v4d acc[Tri<T>::NT];
  unsigned long long tt[4] = {0, 0, 0, 0};
  double cs = 0;
  for (int r = 0; r < reps; ++r) {
    acc_init<T>(k, acc);
#pragma unroll
    for (int K = 0; K < T; ++K) {   // make it safely positive definite: add 20 to the diagonal
#pragma unroll
      for (int p = 0; p < 4; ++p) if (k.q + 4 * p == k.c) acc[Tri<T>::idx(K, K)][p] += 20.0;
    }
    for (int i = k.lane; i < 16 * T; i += 64) RV[i] = 1.0 + (i & 15);
    __syncthreads();
    __builtin_amdgcn_sched_barrier(0);
    unsigned long long t0 = __builtin_amdgcn_s_memtime();
    reg_factor<T, 1>(k, acc, YL, 1e-30);   // (the headline instantiation's form)
    __builtin_amdgcn_sched_barrier(0);
    unsigned long long t1 = __builtin_amdgcn_s_memtime();
    tt[0] += t1 - t0;
    v4d Yk, none = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int K = 0; K < T; ++K) {
#pragma unroll
      for (int p = 0; p < 4; ++p) { Yk[p] = (k.q + 4 * p == k.c) ? 1.0 : 0.0; if (k.q + 4 * p == k.c) acc[Tri<T>::idx(K, K)][p] += 30.0; }
      diag_factor<DiagForm<T, 1>::form>(k, acc[Tri<T>::idx(K, K)], Yk, none, 1e-30);
      cs += Yk[0];
    }
    __builtin_amdgcn_sched_barrier(0);
    unsigned long long t2 = __builtin_amdgcn_s_memtime();
    tt[1] += t2 - t1;
#pragma unroll
    for (int K = 0; K < T; ++K) { tile_store(k, YL + K * 272, acc[Tri<T>::idx(K, K)]); __syncthreads(); acc[Tri<T>::idx(K, K)] = tile_load_t(k, YL + K * 272); }
    __builtin_amdgcn_sched_barrier(0);
    unsigned long long t3 = __builtin_amdgcn_s_memtime();
    tt[2] += t3 - t2;
    double y[T][4];
    vec_forward<T, true>(k, acc, YL, RV, y);
    WAVE_SYNC();
    vec_backward<T, true>(k, acc, YL, y, RV);
    WAVE_SYNC();
    __builtin_amdgcn_sched_barrier(0);
    unsigned long long t4 = __builtin_amdgcn_s_memtime();
    tt[3] += t4 - t3;
#pragma unroll
    for (int K = 0; K < T; ++K) cs += RV[16 * K + k.c] + acc[Tri<T>::idx(K, K)][1];
  }
  cs = wave_sum(cs);
  if (k.lane == 0) { for (int i = 0; i < 4; ++i) P.dump[(size_t)b * 8 + i] = (double)tt[i] / reps; P.dump[(size_t)b * 8 + 4] = cs; }
}
