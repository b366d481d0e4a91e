// qp_solve_kernel.h -- the one-wavefront-per-QP solve kernel: what translation units 1..4 of qp_solver.hip compile (the main unit
// reads it for the self tests and the probes).  Data layout: qp_solver.hip.  The arithmetic of a row and the decisions of an
// iteration and of the refinement (weights, directions, ratio tests, sigma, step length, merit, exits, acceptance) are qp_rules.h's,
// shared with the workgroup kernel: this file moves the data and reduces across lanes.
#pragma once
#include "qp_solver.h"
#include "qp_lane.h"
#include "qp_rules.h"

// 1: the two right-hand sides of an iteration's factor go through the triangular solves together (A/B builds; the shipped build
// solves them one after the other: profiles/lane_reduce/README.md)
#ifndef QP_SOLVE_PAIR
#define QP_SOLVE_PAIR 0
#endif
// 1: diag_factor builds its MFMA A operand with lane selects on constant masks and updates the diagonal tile first; 0: the former
// form (divergent regions, diagonal tile last).  Same arithmetic, same bits (profiles/chol_panels/README.md).  The choice is made
// per instantiation in DiagForm<T, NB>; the former form is always compiled as the reference of fsaempc_selftest_diag_factor().
#ifndef QP_DIAG_FLAT
#define QP_DIAG_FLAT 1
#endif
// 1: pass 1 keeps the accumulator tiles of M in AGPRs across the trips of a phase where SyrkPin<T, NB> allows it; 0: the former
// code in every instantiation (A/B builds; profiles/syrk_agpr/README.md)
#ifndef QP_SYRK_PIN
#define QP_SYRK_PIN 1
#endif
// 1: the former start-up, v = G x and A~'w of the initial multipliers as two passes (A/B and stamp builds: profiles/startup/README.md)
#ifndef QP_STARTUP_ATW
#define QP_STARTUP_ATW 0
#endif
// slots per load batch of the iteration's row sweeps where SweepBatch<T, NB> does not hold an instantiation at 2 (A/B builds: 2 is
// the former pairwise sweep; profiles/row_sweeps/README.md)
#ifndef QP_SWEEP_BATCH
#define QP_SWEEP_BATCH 6
#endif

namespace {

template <int T> struct Tri {
  static constexpr int NT = T * (T + 1) / 2;
  __host__ __device__ static constexpr int idx(int I, int J) { return I * T - (I * (I - 1)) / 2 + (J - I); }
};

// ---------------------------------------------------------------------------------------------
// solve kernel
// ---------------------------------------------------------------------------------------------
struct Ctx {
  int n, m, T, Kq, J, JB, JT, np, lane, c, q, nc, nb, ntr;
  const int* perm; const int* tcs; const int* aoff; const int* tend;   // row order and operand-stream directory (qp_prep_kernel)
  const double* Aw; const double* Hw; const double* Ab; const double* Hb;
  double* rows;  // base of owner-layout row arrays
  double* ring;  // LDS: operand ring of the streaming passes (records of 1 KB)
  double* cof;   // LDS: per-slot coefficient staging of the streaming passes ([array][64])
  int rowlen;
  double* vec;   // LDS n-vectors, np each
};
// (enum RowArr: qp_solver.h, shared with the workgroup kernel)
enum VecArr { V_X = 0, V_G, V_HX, V_R1, V_R2, V_P1, V_P2, V_P3, V_DX, V_E, V_NARR };   // + 4 border-column vectors MB[b] behind them

DEVINL double* rowp(const Ctx& k, int arr) { return k.rows + (size_t)arr * k.rowlen; }
DEVINL double* vecp(const Ctx& k, int arr) { return k.vec + arr * k.np; }
// An LDS n-vector element read as LDS, for the one place where a row array (global) or an n-vector feeds the same value: left as
// two generic loads the compiler merges them into one flat load of a selected pointer, whose LDS aperture copy the register allocator
// may place in vcc -- which this compiler expands into an illegal instruction (seen in the -O1 guard build).
DEVINL double vec_read(const double* p) { return *(const __attribute__((address_space(3))) double*)p; }

DEVINL bool row_valid(const Ctx& k, int js) {
  if (js < k.J) { const int s = 16 * js + k.c; return s < k.Kq && 4 * s + k.q < k.m; }
  return (js - k.J) * 64 + k.lane < k.n;
}

// Hx through the full symmetric tile grid; the loads of tile row I+1 are in flight while row I is consumed.
// (Fusing this with the accumulator initialisation was measured 5x slower: the unrolled form spills.)
template <int T> DEVINL void hx_tiles(const Ctx& k, const double* X, double* HX) {
  double hx[T], hn[T][4], hc[T][4];
#pragma unroll
  for (int t = 0; t < T; ++t) hx[t] = 0.0;
#pragma unroll
  for (int Jt = 0; Jt < T; ++Jt)
#pragma unroll
    for (int p = 0; p < 4; ++p) hn[Jt][p] = k.Hw[((size_t)Jt * 4 + p) * 64 + k.lane];
#pragma unroll 1
  for (int I = 0; I < T; ++I) {
#pragma unroll
    for (int Jt = 0; Jt < T; ++Jt)
#pragma unroll
      for (int p = 0; p < 4; ++p) hc[Jt][p] = hn[Jt][p];
    if (I + 1 < T) {
#pragma unroll
      for (int Jt = 0; Jt < T; ++Jt)
#pragma unroll
        for (int p = 0; p < 4; ++p) hn[Jt][p] = k.Hw[((size_t)((I + 1) * T + Jt) * 4 + p) * 64 + k.lane];
    }
    double xk[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) xk[p] = X[16 * I + k.q + 4 * p];
#pragma unroll
    for (int Jt = 0; Jt < T; ++Jt)
#pragma unroll
      for (int p = 0; p < 4; ++p) hx[Jt] = fma(hc[Jt][p], xk[p], hx[Jt]);
  }
#pragma unroll
  for (int t = 0; t < T; ++t) {
    double v = q_sum(hx[t]);
    if (k.q == 0) HX[16 * t + k.c] = v;
  }
}
// accumulator initialisation acc = H~ (upper tiles, C/D layout)
template <int T> DEVINL void acc_init(const Ctx& k, v4d* acc) {
#pragma unroll
  for (int I = 0; I < T; ++I)
#pragma unroll
    for (int Jt = I; Jt < T; ++Jt) {
      const double* hp = k.Hw + ((size_t)(I * T + Jt) * 4) * 64 + k.lane;
      v4d h;
#pragma unroll
      for (int p = 0; p < 4; ++p) h[p] = hp[p * 64];
      acc[Tri<T>::idx(I, Jt)] = h;
    }
}

// H~x of the core from the freshly initialised accumulators (the upper tiles of H~ that pass 1 is about to add A'DA to), so the
// 51 KB of H~ are read once per iteration instead of twice.  Tile (I,J), I <= J, in accumulator layout gives (H_IJ' x_I)[c] for
// block J with four FMAs and, for I < J, (H_IJ x_J)[q+4p] for block I with four more; the lane-group / DPP-row sums are taken
// once per block, not per tile.  XV, HX: LDS vectors.
template <int T> DEVINL void hx_from_acc(const Ctx& k, const v4d* acc, const double* XV, double* HX) {
  double xr[T][4], xc[T], sc[T], sr[T][4];
#pragma unroll
  for (int I = 0; I < T; ++I) {
    xc[I] = XV[16 * I + k.c]; sc[I] = 0.0;
#pragma unroll
    for (int p = 0; p < 4; ++p) { xr[I][p] = XV[16 * I + k.q + 4 * p]; sr[I][p] = 0.0; }
  }
#pragma unroll
  for (int I = 0; I < T; ++I)
#pragma unroll
    for (int J = I; J < T; ++J) {
      const v4d& h = acc[Tri<T>::idx(I, J)];
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        sc[J] = fma(h[p], xr[I][p], sc[J]);                 // column form: this lane group's rows of (H_IJ' x_I)[c]
        if (J > I) sr[I][p] = fma(h[p], xc[J], sr[I][p]);   // row form: this lane's column of (H_IJ x_J)[q+4p]
      }
    }
  WAVE_SYNC();
#pragma unroll
  for (int J = 0; J < T; ++J) { const double v = q_sum(sc[J]); if (k.q == 0) HX[16 * J + k.c] = v; }
  WAVE_SYNC();
#pragma unroll
  for (int I = 0; I < T - 1; ++I) {
    grp16_sum(sr[I]);
#pragma unroll
    for (int p = 0; p < 4; ++p) if (k.c == 0) HX[16 * I + k.q + 4 * p] += sr[I][p];
  }
}

// ---------------------------------------------------------------------------------------------
// Operand stream of the passes over A~.  The stream is a plain sequence of 1 KB records (one column tile of one pair of
// k-steps) in exactly the order the passes consume it, so the producer is a linear walk: records go global memory -> LDS by
// `global_load_lds_dwordx4` (no VGPRs involved, LDS address = M0 + lane*16) into a ring of R = D + T records; the consumer
// reads a record with one ds_read_b128 per lane.  The compiler does not track LDS-DMA -> ds_read dependences, so the ordering is
// explicit: the asm memory clobber of the wait keeps the compiler from moving LDS reads or DMA issues across it.
//
// Lead of D = 2T records (two pairs of k-steps at the full tile count, more in the sparse early trips) behind a COUNTED wait:
// a pair's C records are consumed after C new ones have been issued and `s_waitcnt vmcnt(D)` says that at most D vector-memory
// operations are still outstanding.  Loads (LDS-DMA, global, scratch) return in issue order, so the D newest outstanding loads
// are never this pair's; stores may retire in any order, which can only make the wait longer, never shorter.  (One pair of lead
// behind a full drain left passes 2 and 3 waiting on the DMA: their VALU work per pair is shorter than the latency.  The wrong
// iterates of some -O2/-O3 builds were NOT a ring hazard: DESIGN.md, "Build-variant fragility: root cause".)
//
// ONE Stream object per kernel invocation, taken by reference by every pass.  open() reads the phase ends tend[0..T] of the stream
// directory once, before the kernel's first store, as scalar loads; read inside a pass they are vector loads (the kernel has
// stored to global memory by then, the compiler may no longer treat the directory as unclobbered), and the wait for an ordinary
// load in a loop that issues LDS-DMA is a full `vmcnt(0)`: five drains of the ring per pass (1 % of the headline solve kernel).
//
// Every pass restarts at record 0 with an empty ring (start() issues D records), the producer runs up to D records past the end
// of the stream (still inside this QP's workspace) and finish() drains those dead loads before the pass returns.  close() is the
// full drain before the wave ends: no LDS-DMA may land in LDS that has been handed to another workgroup.
// ---------------------------------------------------------------------------------------------
template <int T> struct StreamCfg {
  static constexpr int D = 2 * T;
  static constexpr int R = D + T;
};
template <int T> struct Stream {
  static constexpr int D = StreamCfg<T>::D, R = StreamCfg<T>::R;
  static_assert(R == QP_SOLVE_RING(T), "qp_solve_lds (qp_solver.h) sizes the ring");
  const char* gnext; int slot_i, slot_e;   // wave-uniform producer / consumer state: next global address, ring slots to issue into / consume from
  int tend[T + 1];   // phase ends of the stream directory (tend[C] = number of trips with at most C tiles), read once
  DEVINL void issue(const Ctx& k) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gnext + k.lane * 16),
                                     (__attribute__((address_space(3))) void*)(k.ring + slot_i * 128), 16, 0, 0);
    gnext += 1024;
    slot_i = slot_i + 1 == R ? 0 : slot_i + 1;
  }
  DEVINL void open(const Ctx& k) {   // once per kernel invocation, before the first pass
    gnext = reinterpret_cast<const char*>(k.Aw); slot_i = 0; slot_e = 0;
#pragma unroll
    for (int C = 0; C <= T; ++C) tend[C] = uni(k.tend[C]);
  }
  // Top of a pass.  Called on EVERY path into the pass, an empty stream (ntr == 0) included: the state has come through loops whose
  // exits depend on cross-lane reductions, the compiler takes it for divergent, and one path on which it is not made uniform again
  // puts it -- and the address and slot arithmetic of every record -- into vector registers.
  DEVINL void start(const Ctx& k) {
    gnext = reinterpret_cast<const char*>(k.Aw); slot_i = 0; slot_e = 0;
    if (k.ntr > 0) {
#pragma unroll
      for (int j = 0; j < D; ++j) issue(k);
    }
#pragma unroll
    for (int C = 0; C <= T; ++C) tend[C] = uni(tend[C]);
  }
  template <int C> DEVINL void next_pair(const Ctx& k, v2d* b) {
#pragma unroll
    for (int t = 0; t < C; ++t) issue(k);
    asm volatile("s_waitcnt vmcnt(%0)" :: "n"(D) : "memory");
#pragma unroll
    for (int t = 0; t < C; ++t) {
      int sl = slot_e + t; if (sl >= R) sl -= R;
      b[t] = *reinterpret_cast<const v2d*>(k.ring + sl * 128 + k.lane * 2);
    }
    slot_e += C; if (slot_e >= R) slot_e -= R;
  }
  DEVINL void finish() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }   // end of a pass (ntr > 0)
  DEVINL void close() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
};

// Per-row coefficients of a pass (owner layout [slot][64] in global memory): one slot (16 k-steps) at a time is staged
// in LDS -- NA wave-wide loads per 16 k-steps instead of NA broadcast loads per k-step -- and read back as 16-byte
// pairs (both k-steps of a pair) with the lane group's row as address.
template <int NA> struct CoefStage {
  double reg[NA > 0 ? NA : 1];
  DEVINL void load(const Ctx& k, const double* const* arr, int js) {
    const int jc = js < k.J ? js : k.J - 1;
#pragma unroll
    for (int a = 0; a < NA; ++a) reg[a] = arr[a][jc * 64 + k.lane];
  }
  DEVINL void commit(const Ctx& k) {   // registers -> LDS (the previous slot is dead by now)
#pragma unroll
    for (int a = 0; a < NA; ++a) k.cof[a * 64 + k.lane] = reg[a];
  }
  DEVINL void read_pair(const Ctx& k, int s, v2d* out) const {   // s even: k-steps s, s+1 of lane group q
#pragma unroll
    for (int a = 0; a < NA; ++a) out[a] = *reinterpret_cast<const v2d*>(k.cof + a * 64 + k.q * 16 + (s & 15));
  }
};

// Where the accumulator tiles of M live during pass 1.  The MFMAs take them in AGPRs, the rest of the iteration reads them from
// VGPRs, and left alone the register allocator moves the tiles a phase accumulates into VGPR -> AGPR at the top of every trip and
// back behind the trip's last MFMA (4 C (C+1) moves each way in phase C; the way back waits for that MFMA, so the matrix pipe
// drains once per trip).  An empty asm statement with the tile as an "a" operand in front of a phase's trip loop, at the head of
// the trip body and behind the loop makes the AGPR copy the loop-carried one: it emits no instruction and changes no operand of an
// MFMA or FMA, and every tile goes to the AGPRs once per pass, in front of the first phase that reaches it.  At the head of the
// body alone the moves stay (tiles of the phase) or gather in the first phase's loop (every tile of M): profiles/syrk_agpr/README.md.
// An instantiation that this costs scratch, spilled vector registers or its second wave per SIMD keeps the former code: <3,4>, which
// would go from 0 to 8 spilled vector registers; the others are level or better (profiles/syrk_agpr/resource_usage.txt).
template <int T, int NB> struct SyrkPin { static constexpr bool on = QP_SYRK_PIN && !(T == 3 && NB == 4); };
template <int T, int NB, int C> DEVINL void syrk_pin_tiles(v4d* acc) {   // the tiles phase C reaches: (I, J), I <= J < C
  if constexpr (SyrkPin<T, NB>::on) {
#pragma unroll
    for (int I = 0; I < C; ++I)
#pragma unroll
      for (int Jt = I; Jt < C; ++Jt) asm volatile("" : "+a"(acc[Tri<T>::idx(I, Jt)]));
  }
}

// pass 1: acc += A~' D A~ on the matrix cores; p1 = A~'w1, p2 = A~'w2, p3 = A~'w3 on the VALU beside them.
// The stream is walked trip by trip (4 k-steps); a trip with tc column tiles only touches the tc(tc+1)/2 accumulator
// tiles it can reach.  Trips are sorted by tc, so the pass is T phases with compile-time tile counts (phase C: all
// trips with tc == C) and no branches inside a trip.
template <int T, int NB> DEVINL void pass_syrk(const Ctx& k, Stream<T>& st, v4d* acc, double* P1, double* P2, double* P3, double* MB) {
  constexpr int NBB = NB > 0 ? NB : 1;
  constexpr int NA = 4 + NB;
  const int JS = k.J * 64;
  const double* arr[NA];
  arr[0] = rowp(k, R_D); arr[1] = rowp(k, R_W1); arr[2] = rowp(k, R_W2); arr[3] = rowp(k, R_W3);
#pragma unroll
  for (int e = 0; e < NB; ++e) arr[4 + e] = k.Ab + (size_t)e * JS;
  double p1[T], p2[T], p3[T];
  double pb[NBB][T], sbb[NBB][NBB], pwb[3][NBB];   // border: column of A'DA, border block, border entries of p1..p3
#pragma unroll
  for (int t = 0; t < T; ++t) { p1[t] = 0; p2[t] = 0; p3[t] = 0; }
#pragma unroll
  for (int e = 0; e < NBB; ++e) {
#pragma unroll
    for (int t = 0; t < T; ++t) pb[e][t] = 0;
#pragma unroll
    for (int f = 0; f < NBB; ++f) sbb[e][f] = 0;
    pwb[0][e] = pwb[1][e] = pwb[2][e] = 0;
  }
  CoefStage<NA> cs;
  int tr = 0;
  st.start(k);
  if (k.ntr > 0) cs.load(k, arr, 0);
  auto phase = [&](auto Cc) __attribute__((always_inline)) {
    constexpr int C = decltype(Cc)::value;
    const int tr_end = st.tend[C];
    syrk_pin_tiles<T, NB, C>(acc);
    for (; tr < tr_end; ++tr) {
      syrk_pin_tiles<T, NB, C>(acc);
      if ((tr & 3) == 0) { cs.commit(k); cs.load(k, arr, (tr >> 2) + 1); }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        v2d b[C], cf[NA];
        st.template next_pair<C>(k, b);
        cs.read_pair(k, 4 * tr + 2 * u, cf);
        asm volatile("" ::: "memory");
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          double a[C], ab[NBB];
          const double dd = cf[0][h], w1 = cf[1][h], w2 = cf[2][h], w3 = cf[3][h];
#pragma unroll
          for (int e = 0; e < NB; ++e) ab[e] = cf[4 + e][h];
#pragma unroll
          for (int t = 0; t < C; ++t) a[t] = dd * b[t][h];
#pragma unroll
          for (int I = 0; I < C; ++I)
#pragma unroll
            for (int Jt = I; Jt < C; ++Jt)
              acc[Tri<T>::idx(I, Jt)] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[I], b[Jt][h], acc[Tri<T>::idx(I, Jt)], 0, 0, 0);
#pragma unroll
          for (int t = 0; t < C; ++t) {
            p1[t] = fma(w1, b[t][h], p1[t]); p2[t] = fma(w2, b[t][h], p2[t]); p3[t] = fma(w3, b[t][h], p3[t]);
          }
#pragma unroll
          for (int e = 0; e < NB; ++e) {
            const double dab = dd * ab[e];
#pragma unroll
            for (int t = 0; t < C; ++t) pb[e][t] = fma(dab, b[t][h], pb[e][t]);
#pragma unroll
            for (int f = e; f < NB; ++f) sbb[e][f] = fma(dab, ab[f], sbb[e][f]);
            pwb[0][e] = fma(w1, ab[e], pwb[0][e]); pwb[1][e] = fma(w2, ab[e], pwb[1][e]); pwb[2][e] = fma(w3, ab[e], pwb[2][e]);
          }
        }
      }
    }
    syrk_pin_tiles<T, NB, C>(acc);
  };
  if constexpr (T >= 1) phase(IC<1>{});
  if constexpr (T >= 2) phase(IC<2>{});
  if constexpr (T >= 3) phase(IC<3>{});
  if constexpr (T >= 4) phase(IC<4>{});
  if constexpr (T >= 5) phase(IC<5>{});
  if constexpr (T >= 6) phase(IC<6>{});
  if constexpr (T >= 7) phase(IC<7>{});
  if constexpr (T >= 8) phase(IC<8>{});
  if (k.ntr > 0) st.finish();
#pragma unroll
  for (int t = 0; t < T; ++t) {
    double v1 = q_sum(p1[t]), v2 = q_sum(p2[t]), v3 = q_sum(p3[t]);
    if (k.q == 0) { P1[16 * t + k.c] = v1; P2[16 * t + k.c] = v2; P3[16 * t + k.c] = v3; }
  }
#pragma unroll
  for (int e = 0; e < NB; ++e) {
#pragma unroll
    for (int t = 0; t < T; ++t) { const double vb = q_sum(pb[e][t]); if (k.q == 0) MB[e * k.np + 16 * t + k.c] = vb; }
    // border scalars are identical on the 16 lanes of a group: sum the four groups, lane 0 writes
    const double v1 = q_sum(pwb[0][e]), v2 = q_sum(pwb[1][e]), v3 = q_sum(pwb[2][e]);
    if (k.lane == 0) { P1[k.nc + e] = v1; P2[k.nc + e] = v2; P3[k.nc + e] = v3; }
#pragma unroll
    for (int f = 0; f < NB; ++f) {
      const double sv = q_sum(f >= e ? sbb[e][f] : sbb[f][e]);
      if (k.lane == 0) MB[e * k.np + k.nc + f] = sv;
    }
  }
}

// y = A~ v for NVEC vectors (LDS n-vectors) -> owner-layout row arrays.  FUSE: the first vector is the affine
// direction; as soon as a row's va = a_r' dxa is reduced, the second-order weight
//   w_r = (va+a1)(b1 + c1 (va+a1)) - (a2-va)(b2 + c2 (a2-va))      (a,b,c: per-row coefficients of row phase 1)
// is formed and p_cor += w_r a_r is accumulated in the same pass (saves one full stream over A per iteration).
// FUSE 3 is the polish step (see the kernel).  FUSE -1 is the start-up pass: beside y it accumulates Pcor = A~' w for the row array
// R_W3 (the initial multipliers), with the FMAs of a lane in the order of pass_Atw below, so the initial point costs one pass over
// A~ instead of two.  Same operand stream and phase structure as pass 1.
template <int T, int NB, int NVEC, int FUSE> DEVINL void pass_Av(const Ctx& k, Stream<T>& st, const double* const* vin, double* const* rout, double* Pcor, double* Pcor2 = nullptr, const double* const* cfarr = nullptr) {
  constexpr int NBB = NB > 0 ? NB : 1;
  constexpr int NC = FUSE == 1 ? 6 : (FUSE >= 2 ? 3 : (FUSE == -1 ? 1 : 0));   // per-row coefficient arrays of the fused part
  constexpr int NA = NC + NB;
  const int JS = k.J * 64;
  const double* arr[NA > 0 ? NA : 1];
  if (FUSE == 1) { arr[0] = rowp(k, R_RPL); arr[1] = rowp(k, R_CB1); arr[2] = rowp(k, R_CC1); arr[3] = rowp(k, R_RPU); arr[4] = rowp(k, R_CB2); arr[5] = rowp(k, R_CC2); }
  if (FUSE == -1) arr[0] = rowp(k, R_W3);
  if (FUSE >= 2) { arr[0] = cfarr ? cfarr[0] : rowp(k, R_CB1); arr[1] = cfarr ? cfarr[1] : rowp(k, R_RPL); arr[2] = cfarr ? cfarr[2] : rowp(k, R_CC1); }   // refinement: rho*act, target b, multiplier y
#pragma unroll
  for (int f = 0; f < NB; ++f) arr[NC + f] = k.Ab + (size_t)f * JS;
  double v[NVEC][T], vb[NVEC][NBB], pc[T], pcb[NBB], pd[FUSE >= 2 ? T : 1], pdb[NBB];
#pragma unroll
  for (int e = 0; e < NVEC; ++e) {
#pragma unroll
    for (int t = 0; t < T; ++t) v[e][t] = vin[e][16 * t + k.c];
#pragma unroll
    for (int f = 0; f < NB; ++f) vb[e][f] = vin[e][k.nc + f];
  }
#pragma unroll
  for (int t = 0; t < T; ++t) pc[t] = 0.0;
#pragma unroll
  for (int f = 0; f < NBB; ++f) { pcb[f] = 0.0; pdb[f] = 0.0; }
#pragma unroll
  for (int t = 0; t < (FUSE >= 2 ? T : 1); ++t) pd[t] = 0.0;
  double keep[NVEC + 1];   // last entry: the updated multiplier of the polish modes (written to rout[NVEC])
#pragma unroll
  for (int e = 0; e < NVEC + 1; ++e) keep[e] = 0.0;
  CoefStage<NA> cs;
  int tr = 0;
  st.start(k);
  if (k.ntr > 0 && NA > 0) cs.load(k, arr, 0);
  auto phase = [&](auto Cc) __attribute__((always_inline)) {
    constexpr int C = decltype(Cc)::value;
    const int tr_end = st.tend[C];
    for (; tr < tr_end; ++tr) {
      if (NA > 0 && (tr & 3) == 0) { cs.commit(k); cs.load(k, arr, (tr >> 2) + 1); }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        v2d b[C], cf[NA > 0 ? NA : 1];
        st.template next_pair<C>(k, b);
        if (NA > 0) cs.read_pair(k, 4 * tr + 2 * u, cf);
        asm volatile("" ::: "memory");
        double ds[2 * NVEC];   // the two k-steps times the NVEC vectors: independent row sums, reduced as one batch
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int e = 0; e < NVEC; ++e) {
            double a = 0.0;
#pragma unroll
            for (int t = 0; t < C; ++t) a = fma(b[t][h], v[e][t], a);
            ds[h * NVEC + e] = a;
          }
        grp16_sum(ds);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int s = 4 * tr + 2 * u + h;
          const int cc = s & 15;
#pragma unroll
          for (int e = 0; e < NVEC; ++e) {
            double dsum = ds[h * NVEC + e];
#pragma unroll
            for (int f = 0; f < NB; ++f) dsum = fma(cf[NC + f][h], vb[e][f], dsum);
            if (k.c == cc) keep[e] = dsum;
            if (FUSE >= 2 && e == 0) {   // polish: pen = rho*act*(v - b), y^ = y - pen; accumulate A~'y^ and A~'pen
              const double pen = cf[0][h] * (dsum - cf[1][h]);
              const double ynew = cf[2][h] - pen;
              if (k.c == cc) keep[NVEC] = ynew;
#pragma unroll
              for (int t = 0; t < C; ++t) { pc[t] = fma(ynew, b[t][h], pc[t]); pd[t] = fma(pen, b[t][h], pd[t]); }
#pragma unroll
              for (int f = 0; f < NB; ++f) { pcb[f] = fma(ynew, cf[NC + f][h], pcb[f]); pdb[f] = fma(pen, cf[NC + f][h], pdb[f]); }
            }
            if (FUSE == 1 && e == 0) {
              const double dl_ = dsum + cf[0][h], du_ = cf[3][h] - dsum;
              const double w = dl_ * fma(cf[2][h], dl_, cf[1][h]) - du_ * fma(cf[5][h], du_, cf[4][h]);
#pragma unroll
              for (int t = 0; t < C; ++t) pc[t] = fma(w, b[t][h], pc[t]);
#pragma unroll
              for (int f = 0; f < NB; ++f) pcb[f] = fma(w, cf[NC + f][h], pcb[f]);
            }
            if (FUSE == -1 && e == 0) {
              const double w = cf[0][h];
#pragma unroll
              for (int t = 0; t < C; ++t) pc[t] = fma(w, b[t][h], pc[t]);
#pragma unroll
              for (int f = 0; f < NB; ++f) pcb[f] = fma(w, cf[NC + f][h], pcb[f]);
            }
          }
          if (cc == 15 || s + 1 == 4 * k.ntr) {
            const int js = s >> 4;
#pragma unroll
            for (int e = 0; e < NVEC; ++e) { rout[e][js * 64 + k.lane] = keep[e]; keep[e] = 0.0; }
            if (FUSE >= 2) { rout[NVEC][js * 64 + k.lane] = keep[NVEC]; keep[NVEC] = 0.0; }
          }
        }
      }
    }
  };
  if constexpr (T >= 1) phase(IC<1>{});
  if constexpr (T >= 2) phase(IC<2>{});
  if constexpr (T >= 3) phase(IC<3>{});
  if constexpr (T >= 4) phase(IC<4>{});
  if constexpr (T >= 5) phase(IC<5>{});
  if constexpr (T >= 6) phase(IC<6>{});
  if constexpr (T >= 7) phase(IC<7>{});
  if constexpr (T >= 8) phase(IC<8>{});
  if (k.ntr > 0) st.finish();
  if (FUSE) {
#pragma unroll
    for (int t = 0; t < T; ++t) {
      double pv = q_sum(pc[t]);
      if (k.q == 0) Pcor[16 * t + k.c] = pv;
    }
#pragma unroll
    for (int f = 0; f < NB; ++f) { const double pv = q_sum(pcb[f]); if (k.lane == 0) Pcor[k.nc + f] = pv; }
  }
  if (FUSE >= 2) {
#pragma unroll
    for (int t = 0; t < T; ++t) {
      double pv = q_sum(pd[t]);
      if (k.q == 0) Pcor2[16 * t + k.c] = pv;
    }
#pragma unroll
    for (int f = 0; f < NB; ++f) { const double pv = q_sum(pdb[f]); if (k.lane == 0) Pcor2[k.nc + f] = pv; }
  }
}

// p = A~' w (w: owner-layout row array) -> LDS n-vector.  The kernel no longer calls it (the start-up pass, pass_Av with FUSE -1,
// produces the same bits); it stays as the reference of fsaempc_selftest_initial_point().
template <int T, int NB> DEVINL void pass_Atw(const Ctx& k, const double* W, double* Pout) {
  constexpr int NBB = NB > 0 ? NB : 1;
  const int JS = k.J * 64;
  double p[T], pbv[NBB];
#pragma unroll
  for (int t = 0; t < T; ++t) p[t] = 0.0;
#pragma unroll
  for (int f = 0; f < NBB; ++f) pbv[f] = 0.0;
  for (int s = 0; s < 4 * k.ntr; ++s) {
    const int ri = (s >> 4) * 64 + k.q * 16 + (s & 15);
    const double w = W[ri];
    const int tr = s >> 2, tc = k.tcs[tr];
    const double* src = k.Aw + ((size_t)k.aoff[tr] + ((s >> 1) & 1) * tc) * 128 + k.lane * 2 + (s & 1);
#pragma unroll
    for (int t = 0; t < T; ++t)
      if (t < tc) p[t] = fma(w, src[t * 128], p[t]);
#pragma unroll
    for (int f = 0; f < NB; ++f) pbv[f] = fma(w, k.Ab[(size_t)f * JS + ri], pbv[f]);
  }
#pragma unroll
  for (int t = 0; t < T; ++t) {
    double v = q_sum(p[t]);
    if (k.q == 0) Pout[16 * t + k.c] = v;
  }
#pragma unroll
  for (int f = 0; f < NB; ++f) { const double pv = q_sum(pbv[f]); if (k.lane == 0) Pout[k.nc + f] = pv; }
}

// ---------------------------------------------------------------------------------------------
// Register-resident blocked Cholesky M = U'U on the matrix cores.
//
// A 16x16 tile X held in accumulator (C/D) layout -- lane (c,q), reg p <-> X[q+4p][c] -- can be fed straight
// back as an MFMA operand: as the A operand it acts as X' (A[i][k] = X[k][i]), as the B operand as X.  Four
// MFMAs (p = 0..3) therefore compute X'Y for any two resident tiles with no data movement, which is all an
// upper-form blocked Cholesky needs:  U_KJ = U_KK^-T M_KJ (done as row operations on the whole block row),
// M_IJ -= U_KI' U_KJ.  The solves with the factor run on the VALU (vec_forward / vec_backward below).
// ---------------------------------------------------------------------------------------------
template <int T> DEVINL void mfma4_sub(const v4d& X, const v4d& Y, v4d& Dst) {  // Dst -= X' Y
#pragma unroll
  for (int p = 0; p < 4; ++p) Dst = __builtin_amdgcn_mfma_f64_16x16x4f64(-X[p], Y[p], Dst, 0, 0, 0);
}
DEVINL v4d mfma4_new(const v4d& X, const v4d& Y) {  // X' Y
  v4d Z = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int p = 0; p < 4; ++p) Z = __builtin_amdgcn_mfma_f64_16x16x4f64(X[p], Y[p], Z, 0, 0, 0);
  return Z;
}

// resident LDS tiles (row-major, 17-double rows): store once, read back either as stored or transposed
DEVINL void tile_store(const Ctx& k, double* slot, const v4d& Xt) {
#pragma unroll
  for (int p = 0; p < 4; ++p) slot[(k.q + 4 * p) * 17 + k.c] = Xt[p];
}
DEVINL v4d tile_load(const Ctx& k, const double* slot) {
  v4d Z;
#pragma unroll
  for (int p = 0; p < 4; ++p) Z[p] = slot[(k.q + 4 * p) * 17 + k.c];
  return Z;
}
DEVINL v4d tile_load_t(const Ctx& k, const double* slot) {
  v4d Z;
#pragma unroll
  for (int p = 0; p < 4; ++p) Z[p] = slot[k.c * 17 + k.q + 4 * p];
  return Z;
}

// Factorise one 16x16 diagonal tile D = U'U in place, four 4-row panels, and apply the same row operations to two
// companion tiles: Yk (enters as the identity, leaves as U^-T) and rk (leaves as U^-T rk).  The kernel has no use for rk any more
// (the solves run on the VALU): FactorStep hands in a tile of zeros and the compiler drops its operations; the self test still
// compares it between the forms.  Without the parameter the T = 5 bordered kernels are scheduled differently
// (profiles/retire_variants/README.md).  Follow-up: remove it with the next change that alters and
// measures these kernels anyway.
// Per panel p: the 4x4 diagonal block (10 numbers, read with v_readlane) is factorised and inverted redundantly by
// every lane -- W = R^-T, wave-uniform -- and applied to the panel rows of the three tiles as one K=4 MFMA each
// (A operand = W scattered to the panel's rows); the rows of the later panels are then updated by one more K=4 MFMA
// per tile.  No cross-lane data movement besides the readlanes, no LDS.  (The former version walked the 16 rows one
// by one with three ds_bpermute round trips per row: 12k cycles per tile, 80 % of the whole factorisation.)
// Only these three tiles see VALU work; every other tile of the factorisation is touched by the matrix cores alone.
// FLAT: each of the ten values of W goes to exactly one lane, and which one is known at compile time, so the operand is a chain of
// selects on constant lane masks (s_mov + 2 v_cndmask per value, no compare result to keep alive, no exec-mask regions); and the
// diagonal tile is updated before its companions, so that the readlanes of the next panel can start under their MFMAs.
DEVINL double on_lanes(unsigned long long mask, double v, double otherwise) {   // mask: wave-uniform (here: constant once unrolled)
  return __builtin_amdgcn_inverse_ballot_w64(mask) ? v : otherwise;
}
template <int FORM> DEVINL int diag_factor(const Ctx& k, v4d& Ud, v4d& Yk, v4d& rk, double floor_abs) {
  constexpr bool FLAT = FORM >= 1;
  int bad = 0;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    // D[a][b] = M[4p+a][4p+b] lives in lane (c = 4p+b, q = a), register p
    const double d00 = rl(Ud[p], 4 * p + 0), d01 = rl(Ud[p], 4 * p + 1), d02 = rl(Ud[p], 4 * p + 2), d03 = rl(Ud[p], 4 * p + 3);
    const double d11 = rl(Ud[p], 16 + 4 * p + 1), d12 = rl(Ud[p], 16 + 4 * p + 2), d13 = rl(Ud[p], 16 + 4 * p + 3);
    const double d22 = rl(Ud[p], 32 + 4 * p + 2), d23 = rl(Ud[p], 32 + 4 * p + 3);
    const double d33 = rl(Ud[p], 48 + 4 * p + 3);
    auto piv = [&](double t) {
      if constexpr (FORM >= 2) {   // the same floor and the same flag, written as selects: the four panels of a tile stay one basic block
        const bool low = !(t > floor_abs);
        bad |= (low & !(fabs(t) < INFINITY)) ? 1 : 0;
        t = low ? floor_abs : t;
      } else {
        if (!(t > floor_abs)) { if (!(fabs(t) < INFINITY)) bad = 1; t = floor_abs; }
      }
      return rsqrt(t);
    };
    // R'R = D (R upper triangular), i_a = 1/R[a][a]
    const double i0 = piv(d00);
    const double r01 = d01 * i0, r02 = d02 * i0, r03 = d03 * i0;
    const double i1 = piv(fma(-r01, r01, d11));
    const double r12 = fma(-r01, r02, d12) * i1, r13 = fma(-r01, r03, d13) * i1;
    const double i2 = piv(fma(-r12, r12, fma(-r02, r02, d22)));
    const double r23 = fma(-r12, r13, fma(-r02, r03, d23)) * i2;
    const double i3 = piv(fma(-r23, r23, fma(-r13, r13, fma(-r03, r03, d33))));
    // W = (R')^-1, lower triangular
    const double w10 = -r01 * i0 * i1;
    const double w20 = -fma(r12, w10, r02 * i0) * i2, w21 = -r12 * i1 * i2;
    const double w30 = -fma(r23, w20, fma(r13, w10, r03 * i0)) * i3, w31 = -fma(r23, w21, r13 * i1) * i3, w32 = -r23 * i2 * i3;
    // A operand: lane (i = c, kq = q) holds W[c-4p][q] on the panel's rows, 0 elsewhere.  (The compiler turns these selects into
    // ~12 divergent regions per panel and sinks the products above into them.  A branch-free construction -- 0/1 masks times the
    // ten values -- was measured in round 2: 34 % fewer instructions in the factorisation, but 464 instead of 79 spilled
    // registers in the kernel and 17 % slower overall; a leaner rsqrt alone was 2 % slower for the same reason.)
    const v4d z = {0.0, 0.0, 0.0, 0.0};
    if constexpr (FLAT) {
      const unsigned long long L0 = 1ull << (4 * p), L1 = 1ull << (16 + 4 * p), L2 = 1ull << (32 + 4 * p), L3 = 1ull << (48 + 4 * p);
      double wa = on_lanes(L0, i0, 0.0);
      wa = on_lanes(L0 << 1, w10, wa); wa = on_lanes(L0 << 2, w20, wa); wa = on_lanes(L0 << 3, w30, wa);
      wa = on_lanes(L1 << 1, i1, wa); wa = on_lanes(L1 << 2, w21, wa); wa = on_lanes(L1 << 3, w31, wa);
      wa = on_lanes(L2 << 2, i2, wa); wa = on_lanes(L2 << 3, w32, wa);
      wa = on_lanes(L3 << 3, i3, wa);
      const v4d nu = __builtin_amdgcn_mfma_f64_16x16x4f64(wa, Ud[p], z, 0, 0, 0);
      Ud[p] = nu[p];
      double a = 0.0;
      if (p < 3) {
        a = on_lanes(0x0001000100010001ull * (0xFFFFull & (0xFFFFull << (4 * p + 4))), -Ud[p], 0.0);   // columns c > 4p + 3
        Ud = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Ud[p], Ud, 0, 0, 0);
      }
      const v4d ny = __builtin_amdgcn_mfma_f64_16x16x4f64(wa, Yk[p], z, 0, 0, 0);
      const v4d nr = __builtin_amdgcn_mfma_f64_16x16x4f64(wa, rk[p], z, 0, 0, 0);
      Yk[p] = ny[p]; rk[p] = nr[p];
      if (p < 3) {
        Yk = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Yk[p], Yk, 0, 0, 0);
        rk = __builtin_amdgcn_mfma_f64_16x16x4f64(a, rk[p], rk, 0, 0, 0);
      }
      if constexpr (FORM >= 2) asm("" : "+v"(bad));   // the flag is settled per panel: no compare mask or pivot outlives its panel
    } else {
      const int a_ = k.c - 4 * p;
      double wa = 0.0;
      if (k.q == 0) wa = a_ == 0 ? i0 : (a_ == 1 ? w10 : (a_ == 2 ? w20 : (a_ == 3 ? w30 : 0.0)));
      if (k.q == 1) wa = a_ == 1 ? i1 : (a_ == 2 ? w21 : (a_ == 3 ? w31 : 0.0));
      if (k.q == 2) wa = a_ == 2 ? i2 : (a_ == 3 ? w32 : 0.0);
      if (k.q == 3) wa = a_ == 3 ? i3 : 0.0;
      const v4d nu = __builtin_amdgcn_mfma_f64_16x16x4f64(wa, Ud[p], z, 0, 0, 0);
      const v4d ny = __builtin_amdgcn_mfma_f64_16x16x4f64(wa, Yk[p], z, 0, 0, 0);
      const v4d nr = __builtin_amdgcn_mfma_f64_16x16x4f64(wa, rk[p], z, 0, 0, 0);
      Ud[p] = nu[p]; Yk[p] = ny[p]; rk[p] = nr[p];
      if (p < 3) {
        const double a = (k.c > 4 * p + 3) ? -Ud[p] : 0.0;
        Yk = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Yk[p], Yk, 0, 0, 0);
        rk = __builtin_amdgcn_mfma_f64_16x16x4f64(a, rk[p], rk, 0, 0, 0);
        Ud = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Ud[p], Ud, 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) if (k.c < k.q + 4 * p) Ud[p] = 0.0;   // strictly lower part only ever held the symmetric copy
  return bad;
}

// Which form of diag_factor an instantiation takes: one that the new form costs registers keeps the former one.  With the shipped
// flags either new form gives <5,0> 20 instead of 8 spilled vector registers, T = 6 and T = 7 more scratch, and T <= 3 ten more
// AGPRs, which takes <2,1> from two waves per SIMD to one (profiles/chol_panels/resource_usage.txt); <5,1> and <5,4> are level
// or better.
template <int T, int NB> struct DiagForm { static constexpr int form = (T == 5 && NB > 0) ? QP_DIAG_FLAT : 0; };

// How many owner-layout slots a row sweep of the iteration (row phase 2, step length, update) loads before it runs their bodies:
// one exposed global round trip per batch instead of one per pair of slots.  The bodies still run in ascending slot order, so the
// sums and the blocking-pair scan are those of the pairwise sweep, bit for bit.  An instantiation that the wider batch costs
// scratch or spilled vector registers keeps the former 2 (profiles/row_sweeps/resource_usage.txt).
template <int T, int NB> struct SweepBatch { static constexpr int nsb = (T == 5 && NB > 0) ? QP_SWEEP_BATCH : 2; };

// Blocked Cholesky of acc (upper tiles) in place.  Yt[K] = U_KK^-T stays in LDS (YL) for the solves.
template <int T, int NB, int K> struct FactorStep {
  static DEVINL int run(const Ctx& k, v4d* acc, double* YL, double floor_abs) {
    v4d Yk, none = {0.0, 0.0, 0.0, 0.0};   // (none: diag_factor's unused second companion)
#pragma unroll
    for (int p = 0; p < 4; ++p) Yk[p] = (k.q + 4 * p == k.c) ? 1.0 : 0.0;
    int bad = diag_factor<DiagForm<T, NB>::form>(k, acc[Tri<T>::idx(K, K)], Yk, none, floor_abs);
    tile_store(k, YL + K * 272, Yk);          // U_KK^-T stays in LDS for the solves of this iteration
    WAVE_SYNC();
    const v4d Wk = tile_load_t(k, YL + K * 272);   // U_KK^-1
    // U_KJ = U_KK^-T M_KJ through the explicit inverse, then one step of refinement against U_KK itself:
    // U_KJ += U_KK^-T (M_KJ - U_KK' U_KJ).  The product with the explicit inverse alone leaves a backward error of
    // cond(U_KK) eps in the block row (measured on the normal matrix of kinematic N = 40 id 6585 at iteration 14,
    // cond(U_00) = 6e7: |M - U'U| / |M| = 1.8e-14 against 1e-15 for a substitution; the refined row reaches 7e-16), which
    // reappears as noise in the dual residual of the next iterate (10x the CPU oracle's) and jams the end game.
    const v4d& UKK = acc[Tri<T>::idx(K, K)];
#pragma unroll
    for (int Jt = K + 1; Jt < T; ++Jt) {
      v4d Rr = acc[Tri<T>::idx(K, Jt)];
      v4d Ukj = mfma4_new(Wk, Rr);
      mfma4_sub<T>(UKK, Ukj, Rr);                                                   // M_KJ - U_KK' U_KJ
#pragma unroll
      for (int p = 0; p < 4; ++p) Ukj = __builtin_amdgcn_mfma_f64_16x16x4f64(Wk[p], Rr[p], Ukj, 0, 0, 0);
      acc[Tri<T>::idx(K, Jt)] = Ukj;
    }
#pragma unroll
    for (int I = K + 1; I < T; ++I) {
      const v4d& UKI = acc[Tri<T>::idx(K, I)];
#pragma unroll
      for (int Jt = I; Jt < T; ++Jt) mfma4_sub<T>(UKI, acc[Tri<T>::idx(K, Jt)], acc[Tri<T>::idx(I, Jt)]);
    }
    return bad | FactorStep<T, NB, K + 1>::run(k, acc, YL, floor_abs);
  }
};
template <int T, int NB> struct FactorStep<T, NB, T> {
  static DEVINL int run(const Ctx&, v4d*, double*, double) { return 0; }
};
template <int T, int NB> DEVINL int reg_factor(const Ctx& k, v4d* acc, double* YL, double floor_abs) {
  return FactorStep<T, NB, 0>::run(k, acc, YL, floor_abs);
}

// ---------------------------------------------------------------------------------------------
// Triangular solves of ONE right-hand side on the VALU.  A 16-wide right-hand-side tile column on the matrix cores spends 16x
// the work on a single vector and chains four dependent 64-cycle MFMAs per tile; the same products here are four FMAs per tile
// plus DPP / lane-swap reductions, and the backward sweep needs no tile transposes through LDS.
// Vector layouts: "by column": lane (c, .) holds v[c];  "by row": reg p of lane (., q) holds v[q + 4p]  (each replicated
// over the other lane coordinate).  Tiles are in accumulator layout: lane (c,q), reg p <-> X[q+4p][c].
// ---------------------------------------------------------------------------------------------
// REFINE: the diagonal blocks are applied through their explicit inverses U_KK^-T (LDS tiles); one step of refinement against
// U_KK itself makes that as accurate as a substitution.  The two step directions of an iteration need it (without it 1 of 4096
// kinematic N = 20 instances diverged), the corrector solve never had it.
// U'y = b:  t_K = b_K - sum_{I<K} U_IK' y_I (by column),  y_K = U_KK^-T t_K (by row).  B: LDS vector (core part).
// NV right-hand sides of one factor are solved together: one tile load per K for all of them and their reductions as one batch
// (NV x 4 independent chains); the operations of each vector and their order are those of a solve of that vector alone.
template <int T, bool REFINE, int NV> DEVINL void vec_forward(const Ctx& k, const v4d* acc, const double* YL, const double* const (&B)[NV], double (&y)[NV][T][4]) {
#pragma unroll
  for (int K = 0; K < T; ++K) {
    double s[NV], t[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      s[v] = 0.0;
#pragma unroll
      for (int I = 0; I < K; ++I)
#pragma unroll
        for (int p = 0; p < 4; ++p) s[v] = fma(acc[Tri<T>::idx(I, K)][p], y[v][I][p], s[v]);   // this lane group's rows of (U_IK' y_I)[c]
    }
    if (K > 0) q_sum(s);
#pragma unroll
    for (int v = 0; v < NV; ++v) t[v] = B[v][16 * K + k.c] - (K > 0 ? s[v] : 0.0);
    const v4d Yt = tile_load(k, YL + K * 272);                                        // U_KK^-T
    double yk[NV * 4];
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int p = 0; p < 4; ++p) yk[4 * v + p] = Yt[p] * t[v];
    grp16_sum(yk);                                                                    // y_K[q+4p] = sum_c Y[q+4p][c] t[c]
    if (REFINE) {
      const v4d& U = acc[Tri<T>::idx(K, K)];
      double r[NV], dy[NV * 4];
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        r[v] = 0.0;
#pragma unroll
        for (int p = 0; p < 4; ++p) r[v] = fma(U[p], yk[4 * v + p], r[v]);
      }
      q_sum(r);
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        r[v] = t[v] - r[v];                                                           // t - U_KK' y  (by column)
#pragma unroll
        for (int p = 0; p < 4; ++p) dy[4 * v + p] = Yt[p] * r[v];
      }
      grp16_sum(dy);
#pragma unroll
      for (int i = 0; i < NV * 4; ++i) yk[i] += dy[i];
    }
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int p = 0; p < 4; ++p) y[v][K][p] = yk[4 * v + p];
  }
}
template <int T, bool REFINE> DEVINL void vec_forward(const Ctx& k, const v4d* acc, const double* YL, const double* B, double (&y)[T][4]) {
  const double* const b1[1] = {B};
  vec_forward<T, REFINE, 1>(k, acc, YL, b1, reinterpret_cast<double (&)[1][T][4]>(y));
}
// U x = y:  w_K = y_K - sum_{J>K} U_KJ x_J (by row),  x_K = U_KK^-1 w_K = (U_KK^-T)' w_K (by column) -> X (LDS vectors, core part)
template <int T, bool REFINE, int NV> DEVINL void vec_backward(const Ctx& k, const v4d* acc, const double* YL, const double (&y)[NV][T][4], double* const (&X)[NV]) {
  double x[NV][T];
#pragma unroll
  for (int K = T - 1; K >= 0; --K) {
    const v4d Yt = tile_load(k, YL + K * 272);
    double w[NV * 4], s[NV * 4], s2[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        s[4 * v + p] = 0.0;
#pragma unroll
        for (int J = K + 1; J < T; ++J) s[4 * v + p] = fma(acc[Tri<T>::idx(K, J)][p], x[v][J], s[4 * v + p]);   // this lane's column of (U_KJ x_J)[q+4p]
      }
    if (K < T - 1) grp16_sum(s);
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      s2[v] = 0.0;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        w[4 * v + p] = y[v][K][p] - (K < T - 1 ? s[4 * v + p] : 0.0);
        s2[v] = fma(Yt[p], w[4 * v + p], s2[v]);
      }
    }
    q_sum(s2);
#pragma unroll
    for (int v = 0; v < NV; ++v) x[v][K] = s2[v];
    if (REFINE) {
      const v4d& U = acc[Tri<T>::idx(K, K)];
      double d[NV], ux[NV * 4];
#pragma unroll
      for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int p = 0; p < 4; ++p) ux[4 * v + p] = U[p] * x[v][K];
      grp16_sum(ux);
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        d[v] = 0.0;
#pragma unroll
        for (int p = 0; p < 4; ++p) d[v] = fma(Yt[p], w[4 * v + p] - ux[4 * v + p], d[v]);   // Y' (w - U_KK x)
      }
      q_sum(d);
#pragma unroll
      for (int v = 0; v < NV; ++v) x[v][K] += d[v];
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) if (k.q == 0) X[v][16 * K + k.c] = x[v][K];
  }
}
template <int T, bool REFINE> DEVINL void vec_backward(const Ctx& k, const v4d* acc, const double* YL, const double (&y)[T][4], double* X) {
  double* const x1[1] = {X};
  vec_backward<T, REFINE, 1>(k, acc, YL, reinterpret_cast<const double (&)[1][T][4]>(y), x1);
}
// by-row vector <-> LDS vector
template <int T> DEVINL void vec_rows_store(const Ctx& k, const double (&y)[T][4], double* V) {
  if (k.c == 0) {
#pragma unroll
    for (int K = 0; K < T; ++K)
#pragma unroll
      for (int p = 0; p < 4; ++p) V[16 * K + k.q + 4 * p] = y[K][p];
  }
}
template <int T> DEVINL void vec_rows_load(const Ctx& k, const double* V, double (&y)[T][4]) {
#pragma unroll
  for (int K = 0; K < T; ++K)
#pragma unroll
    for (int p = 0; p < 4; ++p) y[K][p] = V[16 * K + k.q + 4 * p];
}

#ifndef QP_STAMPS
#define QP_STAMPS 0
#endif
// QP_STAMPS=2 splits the start-up instead of the loop: ids 2, 3, 4 = the v = G x pass, the row initialisation, hx_full; id 0 keeps
// what follows them (the former pass_Atw, the multiplier fix-up) and id 1 takes the whole iteration loop and the epilogue.
#if QP_STAMPS >= 2
#define STAMP(id) STAMP_AT(((id) >= 1) ? 1 : 0)
#define STAMP_SETUP(id) STAMP_AT(id)
#else
#define STAMP(id) STAMP_AT(id)
#define STAMP_SETUP(id) do { } while (0)
#endif
#if QP_STAMPS
#define STAMP_DECL unsigned long long st_acc[16]; for (int i_ = 0; i_ < 16; ++i_) st_acc[i_] = 0; unsigned long long st_t0 = __builtin_amdgcn_s_memtime();
#define STAMP_AT(id) do { __builtin_amdgcn_sched_barrier(0); unsigned long long t_ = __builtin_amdgcn_s_memtime(); st_acc[id] += t_ - st_t0; st_t0 = t_; __builtin_amdgcn_sched_barrier(0); } while (0)
#define STAMP_OUT do { if (P.dump && P.dump_stage == 9 && lane == 0) for (int i_ = 0; i_ < 16; ++i_) P.dump[(size_t)b * 16 + i_] = (double)st_acc[i_]; } while (0)
#else
#define STAMP_DECL
#define STAMP_AT(id) do { } while (0)
#define STAMP_OUT do { } while (0)
#endif

// One QP as the kernel sees it: dimensions, this lane's coordinates, the arrays of the QP's workspace, the LDS base.  k.ring and k.cof
// are the caller's to set: it carves the regions behind the n-vectors with qp_solve_lds.  Returns the QP's workspace.
static_assert(V_NARR == QP_SOLVE_NVEC, "qp_solve_lds (qp_solver.h) counts the n-vectors");
template <int T> DEVINL double* ctx_setup(Ctx& k, const QpParams& P, int b, double* lds) {
  const QpDims& d = P.d;
  k.n = d.n; k.m = d.m; k.T = T; k.Kq = d.Kq; k.J = d.J; k.JB = d.JB; k.JT = d.J + d.JB; k.np = d.np;
  k.lane = threadIdx.x; k.c = k.lane & 15; k.q = k.lane >> 4; k.nc = d.nc; k.nb = d.nb;
  double* ws = P.ws + (size_t)b * d.ws_per_qp;
  k.Aw = ws + d.off_Aw; k.Hw = ws + d.off_Hw; k.Ab = ws + d.off_Ab; k.Hb = ws + d.off_Hb;
  k.rows = ws + d.off_rows; k.rowlen = d.rowlen; k.ntr = d.ntr;
  k.perm = reinterpret_cast<const int*>(ws + d.off_meta); k.tcs = k.perm + (size_t)(d.J > 0 ? d.J : 1) * 64;
  k.aoff = k.tcs + d.ntr; k.tend = k.aoff + d.ntr + 1;
  k.vec = lds;
  return ws;
}

template <int T, int NB> __global__ __launch_bounds__(64, 1) void qp_solve_kernel(QpParams P) {
  const int b = P.order ? P.order[blockIdx.x] : blockIdx.x;   // launch order: hardest-looking instances first
  const QpDims& d = P.d;
  extern __shared__ double lds[];
  Ctx k;
  double* ws = ctx_setup<T>(k, P, b, lds);
  const QpSolveLds L = qp_solve_lds(T, NB, d.np);
  double* MB = lds + L.vecs;      // NB border-column vectors (A'DA border, then U^-T m_b)
  double* YL = MB + L.border;     // T resident tiles U_KK^-T
  k.ring = YL + L.tiles;          // operand ring of the streaming passes
  k.cof = k.ring + L.ring;        // coefficient staging, (6 + NB) arrays of 64
  const double* gw = ws + d.off_gw;
  const double* Es = ws + d.off_E;
  const double* Fs = ws + d.off_F;
  const int lane = k.lane, n = k.n, JT = k.JT, J = k.J, nc = k.nc, nb = k.nb;
  constexpr int NT = Tri<T>::NT;
  constexpr int NBB = NB > 0 ? NB : 1;

#define X vecp(k, V_X)
#define G vecp(k, V_G)
#define HX vecp(k, V_HX)
#define R1 vecp(k, V_R1)
#define R2 vecp(k, V_R2)
#define P1 vecp(k, V_P1)
#define P2 vecp(k, V_P2)
#define P3 vecp(k, V_P3)
#define DX vecp(k, V_DX)
#define EV vecp(k, V_E)
#define aL rowp(k, R_L)
#define aU rowp(k, R_U)
#define aTL rowp(k, R_TL)
#define aTU rowp(k, R_TU)
#define aZL rowp(k, R_ZL)
#define aZU rowp(k, R_ZU)
#define aV rowp(k, R_V)
#define aD rowp(k, R_D)
#define aW1 rowp(k, R_W1)
#define aW2 rowp(k, R_W2)
#define aW3 rowp(k, R_W3)
#define aVA rowp(k, R_VA)
#define aVC rowp(k, R_VC)
#define aRPL rowp(k, R_RPL)
#define aRPU rowp(k, R_RPU)

  // Hx = H~ x: core through the tile grid, border columns (full-length vectors Hb[b]) on the VALU
  auto hx_border = [&](const double* XV) __attribute__((always_inline)) {
    if (NB > 0) {
      WAVE_SYNC();
      double xb[NBB], sb[NBB];
#pragma unroll
      for (int e = 0; e < NB; ++e) { xb[e] = XV[nc + e]; sb[e] = 0.0; }
      for (int h = 0; h < 2; ++h) {
        const int i = lane + 64 * h;
        if (i < n) {
          double add = 0.0;
#pragma unroll
          for (int e = 0; e < NB; ++e) { const double hbi = k.Hb[(size_t)e * k.np + i]; add = fma(hbi, xb[e], add); sb[e] = fma(hbi, XV[i], sb[e]); }
          if (i < nc) HX[i] += add;
        }
      }
      wave_sum(sb);
#pragma unroll
      for (int e = 0; e < NB; ++e) if (lane == 0) HX[nc + e] = sb[e];
    }
  };
  auto hx_full = [&](const double* XV) __attribute__((always_inline)) { hx_tiles<T>(k, XV, HX); hx_border(XV); };

  // the operand stream of every pass of this invocation: its first D records fly while the vectors and bounds are set up
  Stream<T> st;
  st.open(k);

  // ---- load n-vectors, initial x = clamp(0, l, u) (scaled), count finite sides ----
  const double T0 = 10.0, Z0 = 100.0;   // initial slacks / multipliers (below)
  for (int i = lane; i < k.np; i += 64) { G[i] = gw[i]; EV[i] = Es[i]; R1[i] = 0; R2[i] = 0; DX[i] = 0; }
  int cnt_local = 0, infeas = 0;
  for (int js = 0; js < JT; ++js) {
    const int ix = js * 64 + lane;
    const bool valid = row_valid(k, js);
    double l = aL[ix], u = aU[ix];
    if (valid) {
      if (l > -INFINITY && u < INFINITY) {
        if (l > u) infeas = 1;
        if (!(u > l)) {  // equality row: open a tiny interior (documented relaxation)
          const double eps = 1e-9 * fmax(1.0, fabs(l));
          l -= eps; u += eps; aL[ix] = l; aU[ix] = u;
        }
      }
      cnt_local += (l > -INFINITY) + (u < INFINITY);
    }
    // the multipliers of the initial point, z = Z0 on every finite side: the weights of the A~'w that rides on the v = G x pass
    aW3[ix] = (valid && js < J) ? ((l > -INFINITY ? Z0 : 0.0) - (u < INFINITY ? Z0 : 0.0)) : 0.0;
    if (js >= J) {
      const int i = (js - J) * 64 + lane;
      if (i < k.np) {
        double xi = 0.0;
        if (P.x_init) { const int ui = i < k.n ? qp_user_index(d, i) : -1; if (ui >= 0) { const double xs = P.x_init[(size_t)b * d.nu + ui] / EV[i]; if (fabs(xs) < INFINITY) xi = xs; } }
        if (valid) { if (l > -INFINITY && xi < l) xi = l; if (u < INFINITY && xi > u) xi = u; }
        X[i] = xi;
      }
    }
  }
  const double cnt = fmax(1.0, wave_sum((double)cnt_local));
  infeas = wave_max((double)infeas) > 0;
  WAVE_SYNC();

  STAMP_DECL
  int flag = 1, it = 0, flag_polished = 0;
  double fval_s = 0.0, merit_s = INFINITY;   // objective / relative KKT residual of the point that is returned
  if (infeas) { flag = -2; }
  if (ws[d.off_bad] != 0.0) flag = -1;   // NaN / Inf in this QP's data (found by the prep kernel): -1 after 0 iterations, x = clamp(0, lb, ub)

  // ---- v = G x, and P3 = A~'(zl - zu) of the initial multipliers in the same pass ----
  {
    const double* vin[1] = {X}; double* rout[1] = {aV};
#if QP_STARTUP_ATW
    pass_Av<T, NB, 1, 0>(k, st, vin, rout, nullptr);
#else
    pass_Av<T, NB, 1, -1>(k, st, vin, rout, P3);
#endif
    for (int jb = 0; jb < k.JB; ++jb) { const int i = jb * 64 + lane; aV[(J + jb) * 64 + lane] = i < n ? X[i] : 0.0; }
  }
  // ---- initial slacks / multipliers in the equilibrated problem: t = max(resid, T0), z = Z0 (a scan over the
  //      synthetic LTV-MPC families: (10,100) needs 8-16 % fewer iterations than (1,1)) ----
  STAMP_SETUP(2);
  for (int js = 0; js < JT; ++js) {
    const int ix = js * 64 + lane;
    const bool valid = row_valid(k, js);
    const double l = aL[ix], u = aU[ix], v = aV[ix];
    const bool hl = valid && l > -INFINITY, hu = valid && u < INFINITY;
    aTL[ix] = hl ? fmax(v - l, T0) : 1.0;
    aTU[ix] = hu ? fmax(u - v, T0) : 1.0;
    aZL[ix] = hl ? Z0 : 0.0;
    aZU[ix] = hu ? Z0 : 0.0;
  }
  WAVE_SYNC();
  STAMP_SETUP(3);
  // bound multipliers absorb the initial dual residual r = Hx + g - A'(zl - zu)
  {
    hx_full(X);
    STAMP_SETUP(4);
#if QP_STARTUP_ATW   // (A/B and stamp builds of the former start-up: a pass of its own for A~'w)
    pass_Atw<T, NB>(k, aW3, P3);
#endif
    WAVE_SYNC();
    for (int jb = 0; jb < k.JB; ++jb) {
      const int i = jb * 64 + lane, ix = (J + jb) * 64 + lane;
      if (i < n) {
        const double r = HX[i] + G[i] - P3[i];
        if (aL[ix] > -INFINITY) aZL[ix] = fmax(r, 0.0) + Z0;
        if (aU[ix] < INFINITY) aZU[ix] = fmax(-r, 0.0) + Z0;
      }
    }
    WAVE_SYNC();
  }

  // fall-back iterate (best one that met tol_loose)
  double saved_merit = INFINITY, best_res = INFINITY;
  int have_saved = 0, stall = 0;
  double* XS = ws + d.off_save;            // np
  double* LAMS = ws + d.off_save + k.np;   // rowlen

  // residuals and barrier weights of one row (owner lane): everything pass 1 / pass 2 need, in owner layout
  auto row1_body = [&](int ix, bool valid, double l, double u, double v, double tl, double tu, double zl, double zu,
                       double& s_gap, double& m_rp) {
    const QprRow o = qpr_row_weights(valid, l, u, v, tl, tu, zl, zu, s_gap, m_rp);
    aRPL[ix] = o.rpl; aRPU[ix] = o.rpu; rowp(k, R_CB1)[ix] = o.dl; rowp(k, R_CC1)[ix] = o.ccl;
    rowp(k, R_CB2)[ix] = o.du; rowp(k, R_CC2)[ix] = o.ccu;
    aD[ix] = o.D; aW1[ix] = o.W1; aW2[ix] = o.W2; aW3[ix] = o.W3;
  };
  struct Slot { int ix; bool valid; double l, u, v, tl, tu, zl, zu, va, vc, w2, rpl, rpu; };
  auto load_slot = [&](int js) {   // all loads of one owner-layout slot, issued together (one latency per trip)
    Slot s_;
    const int jc = js < JT ? js : JT - 1;
    s_.ix = jc * 64 + lane; s_.valid = js < JT && row_valid(k, jc);
    const int ix = s_.ix;
    s_.l = aL[ix]; s_.u = aU[ix]; s_.v = aV[ix]; s_.tl = aTL[ix]; s_.tu = aTU[ix]; s_.zl = aZL[ix]; s_.zu = aZU[ix];
    s_.va = aVA[ix]; s_.vc = aVC[ix]; s_.w2 = aW2[ix]; s_.rpl = aRPL[ix]; s_.rpu = aRPU[ix];
    return s_;
  };
  // What a variable-bound slot (js >= J) takes from the n-vectors: row `lane` of slot J + h is element i = lane + 64 h, which this
  // very lane holds or reads from LDS, so these values make no trip through the row arrays (whose bound parts of VA, VC, W2 the
  // iteration no longer writes: load_slot's values for them are replaced before a body sees them).
  struct BoundVals { double va[2], vc[2], w2[2]; };
  auto bound_dirs = [&](BoundVals& bv) {   // va, vc of the bound slots: the affine / centering directions in R1, R2
    for (int h = 0; h < 2; ++h) { const int i = lane + 64 * h; bv.va[h] = i < n ? R1[i] : 0.0; bv.vc[h] = i < n ? R2[i] : 0.0; }
  };
  // One row sweep: NSB slots per trip, all their loads issued before the first body runs; slots past JT are clamped and invalid
  // (load_slot), so JT need not be a multiple of NSB.  Bodies run in ascending js.
  constexpr int NSB = SweepBatch<T, NB>::nsb;
  auto sweep = [&](const BoundVals& bv, auto&& body) __attribute__((always_inline)) {
    for (int js0 = 0; js0 < JT; js0 += NSB) {
      Slot r[NSB];
#pragma unroll
      for (int e = 0; e < NSB; ++e) r[e] = load_slot(js0 + e);
#pragma unroll
      for (int e = 0; e < NSB; ++e) {
        const int js = js0 + e;
#pragma unroll
        for (int h = 0; h < 2; ++h)
          if (js == J + h) { r[e].va = bv.va[h]; r[e].vc = bv.vc[h]; r[e].w2 = bv.w2[h]; }
        body(r[e], js);
      }
    }
  };
  double gap = 0.0, rp_rel = 0.0;   // carried across iterations (produced by the update sweep)

  v4d acc[NT];          // upper tiles of M, then of its Cholesky factor U
  double Ubb[NBB][NBB]; // Cholesky factor of the border Schur complement (wave-uniform scalars)
  // border part of a solve: R holds y_c = U^-T b_c (core) and b_b (border); leaves the border solution in R[nc+e]
  // and y_c - sum_e u_e x_e in the core, ready for the backward sweep
  auto border_solve = [&](double* R) __attribute__((always_inline)) {
    if (NB > 0) {
      double yb[NBB], xb[NBB], dsum[NBB];
#pragma unroll
      for (int e = 0; e < NB; ++e) {
        dsum[e] = 0.0;
        for (int h = 0; h < 2; ++h) { const int i = lane + 64 * h; if (i < nc) dsum[e] = fma(MB[e * k.np + i], R[i], dsum[e]); }
      }
      wave_sum(dsum);
#pragma unroll
      for (int e = 0; e < NB; ++e) {
        double tt = R[nc + e] - dsum[e];
#pragma unroll
        for (int g2 = 0; g2 < e; ++g2) tt -= Ubb[g2][e] * yb[g2];
        yb[e] = tt / Ubb[e][e];
      }
#pragma unroll
      for (int e = NB - 1; e >= 0; --e) {
        double tt = yb[e];
#pragma unroll
        for (int f = e + 1; f < NB; ++f) tt -= Ubb[e][f] * xb[f];
        xb[e] = tt / Ubb[e][e];
      }
      WAVE_SYNC();
      for (int h = 0; h < 2; ++h) {
        const int i = lane + 64 * h;
        if (i < nc) {
          double r = R[i];
#pragma unroll
          for (int e = 0; e < NB; ++e) r = fma(-MB[e * k.np + i], xb[e], r);
          R[i] = r;
        }
      }
      if (lane == 0) {
#pragma unroll
        for (int e = 0; e < NB; ++e) R[nc + e] = xb[e];
      }
      WAVE_SYNC();
    }
  };
  // M = (acc from pass 1) + diag(aD on the variable rows), border columns = H~ border + A'DA border (MB); factorise in
  // registers and solve for the two right-hand sides in R1, R2 (in place).  Returns 1 on a non-finite pivot.
  auto factor_solve2 = [&](int it_now) __attribute__((always_inline)) -> int {
    double dmax_l = 0;
#pragma unroll
    for (int K = 0; K < T; ++K) {
      const int i = 16 * K + k.c;                       // diagonal element of tile (K,K) lives on lane c with q = c&3, reg c>>2
      const int ix = (J + (i >> 6)) * 64 + (i & 63);
      const double dadd = i < n ? aD[ix] : 1.0;         // padded indices get a unit diagonal
      const bool mine = (k.q == (k.c & 3));
#pragma unroll
      for (int p = 0; p < 4; ++p)
        if (mine && p == (k.c >> 2)) { acc[Tri<T>::idx(K, K)][p] += dadd; dmax_l = fmax(dmax_l, acc[Tri<T>::idx(K, K)][p]); }
    }
    if (NB > 0) {
      for (int h = 0; h < 2; ++h) {
        const int i = lane + 64 * h;
        if (i < k.np) {
          const int ix = (J + (i >> 6)) * 64 + (i & 63);
#pragma unroll
          for (int e = 0; e < NB; ++e) {   // border column e of M: H~ column + A'DA column (+ its variable-bound weight on the diagonal)
            double v = i < n ? k.Hb[(size_t)e * k.np + i] + MB[e * k.np + i] : 0.0;
            if (i == nc + e) { v += e < nb ? aD[ix] : 1.0; dmax_l = fmax(dmax_l, v); }
            MB[e * k.np + i] = v;
          }
        }
      }
    }
    const double dmax = wave_max(dmax_l);
    WAVE_SYNC();
#ifdef QP_DEBUG_DUMP   // diagnostic build only (libfsaempc_dbg.so): the shipped kernel carries no dump branches
    if (P.dump && b == 0 && P.dump_stage == 1 && it_now == P.dump_iter) {  // debug: M, p1, p2, p3, Hx
#pragma unroll
      for (int I = 0; I < T; ++I)
#pragma unroll
        for (int Jt = I; Jt < T; ++Jt)
#pragma unroll
          for (int p = 0; p < 4; ++p) {
            const int r = 16 * I + k.q + 4 * p, cc = 16 * Jt + k.c;
            if (r < n && cc < n) { P.dump[r * n + cc] = acc[Tri<T>::idx(I, Jt)][p]; if (I != Jt || cc >= r) P.dump[cc * n + r] = acc[Tri<T>::idx(I, Jt)][p]; }
          }
      for (int e = 0; e < nb; ++e)
        for (int i = lane; i < n; i += 64) { P.dump[i * n + nc + e] = MB[e * k.np + i]; P.dump[(nc + e) * n + i] = MB[e * k.np + i]; }
      for (int i = lane; i < n; i += 64) { P.dump[n * n + i] = P1[i]; P.dump[n * n + n + i] = P2[i]; P.dump[n * n + 2 * n + i] = P3[i]; P.dump[n * n + 3 * n + i] = HX[i]; }
    }
#endif
    int fbad = reg_factor<T, NB>(k, acc, YL, 1e-30 * dmax);
    WAVE_SYNC();
    STAMP(5);
    if (NB > 0) {   // bordered factor: u_e = U^-T m_e; S = M_bb - u'u is factorised as scalars
#pragma unroll
      for (int e = 0; e < NB; ++e) {
        double ue[T][4];
        vec_forward<T, true>(k, acc, YL, MB + e * k.np, ue);
        WAVE_SYNC();
        vec_rows_store<T>(k, ue, MB + e * k.np);
      }
      WAVE_SYNC();
      double S[NBB][NBB], ss[NBB * (NBB + 1) / 2];   // the sums of all S[e][f], e <= f, reduced as one batch
#pragma unroll
      for (int e = 0, j = 0; e < NB; ++e)
#pragma unroll
        for (int f = e; f < NB; ++f, ++j) {
          double dsum = 0.0;
          for (int h = 0; h < 2; ++h) { const int i = lane + 64 * h; if (i < nc) dsum = fma(MB[e * k.np + i], MB[f * k.np + i], dsum); }
          ss[j] = dsum;
        }
      wave_sum(ss);
#pragma unroll
      for (int e = 0, j = 0; e < NB; ++e)
#pragma unroll
        for (int f = e; f < NB; ++f, ++j) S[e][f] = MB[e * k.np + nc + f] - ss[j];
#pragma unroll
      for (int e = 0; e < NB; ++e) {
        double dd = S[e][e];
#pragma unroll
        for (int g2 = 0; g2 < e; ++g2) dd -= Ubb[g2][e] * Ubb[g2][e];
        if (!(dd > 1e-30 * dmax)) { if (!(fabs(dd) < INFINITY)) fbad = 1; dd = 1e-30 * dmax; }
        Ubb[e][e] = sqrt(dd);
#pragma unroll
        for (int f = e + 1; f < NB; ++f) {
          double tt = S[e][f];
#pragma unroll
          for (int g2 = 0; g2 < e; ++g2) tt -= Ubb[g2][e] * Ubb[g2][f];
          Ubb[e][f] = tt / Ubb[e][e];
        }
      }
    }
    if (fbad) return 1;
    {
      double y12[2][T][4];
      double (&y1)[T][4] = y12[0], (&y2)[T][4] = y12[1];
#if QP_SOLVE_PAIR
      { const double* const b12[2] = {R1, R2}; vec_forward<T, true, 2>(k, acc, YL, b12, y12); }
#else
      vec_forward<T, true>(k, acc, YL, R1, y1);
      vec_forward<T, true>(k, acc, YL, R2, y2);
#endif
      if (NB > 0) {
        WAVE_SYNC();
        vec_rows_store<T>(k, y1, R1); vec_rows_store<T>(k, y2, R2);
        WAVE_SYNC();
        border_solve(R1); border_solve(R2);
        vec_rows_load<T>(k, R1, y1); vec_rows_load<T>(k, R2, y2);
      }
      WAVE_SYNC();
#if QP_SOLVE_PAIR
      { double* const x12[2] = {R1, R2}; vec_backward<T, true, 2>(k, acc, YL, y12, x12); }
#else
      vec_backward<T, true>(k, acc, YL, y1, R1);
      vec_backward<T, true>(k, acc, YL, y2, R2);
#endif
    }
    WAVE_SYNC();
    return 0;
  };
  // one more solve with the resident factor: V <- M^-1 V (LDS n-vector, in place), on the VALU
  auto solve1 = [&](double* V) __attribute__((always_inline)) {
    double yv[T][4];
    vec_forward<T, false>(k, acc, YL, V, yv);
    if (NB > 0) {
      WAVE_SYNC();
      vec_rows_store<T>(k, yv, V);
      WAVE_SYNC();
      border_solve(V);
      vec_rows_load<T>(k, V, yv);
    }
    WAVE_SYNC();
    vec_backward<T, false>(k, acc, YL, yv, V);
  };

  STAMP(0);
  for (it = 0; flag == 1; ++it) {
    // ================= row phase 1: residuals, weights (only on entry; afterwards fused into the update sweep) =================
    if (it == 0) {
      double s_gap = 0, m_rp = 0;
      for (int js = 0; js < JT; ++js) {
        const int ix = js * 64 + lane;
        row1_body(ix, row_valid(k, js), aL[ix], aU[ix], aV[ix], aTL[ix], aTU[ix], aZL[ix], aZU[ix], s_gap, m_rp);
      }
      gap = wave_sum(s_gap);
      rp_rel = wave_max(m_rp);
      WAVE_SYNC();
    }
    const double mu = gap / cnt;

    STAMP(1);
    // ================= pass 1: M = H + A'DA (MFMA), p1, p2, p3; Hx =================
    acc_init<T>(k, acc);
    hx_from_acc<T>(k, acc, X, HX);
    hx_border(X);
    STAMP(2);
    pass_syrk<T, NB>(k, st, acc, P1, P2, P3, MB);
    WAVE_SYNC();
    STAMP(3);
    // objective, dual residual
    // (the bound rows' weights of the two right-hand sides below are loaded here with W3: one round trip for the block, not two)
    double fl = 0, m_rd = 0, w1b[2] = {0.0, 0.0}, w2b[2] = {0.0, 0.0}, w3b[2] = {0.0, 0.0};
    for (int h = 0; h < 2; ++h) {
      const int i = lane + 64 * h;
      if (i < n) { const int ix = (J + (i >> 6)) * 64 + (i & 63); w3b[h] = aW3[ix]; w1b[h] = aW1[ix]; w2b[h] = aW2[ix]; }
    }
    for (int h = 0; h < 2; ++h) {
      const int i = lane + 64 * h;
      if (i < n) {
        fl += qpr_obj_term(X[i], HX[i], G[i]);
        m_rd = fmax(m_rd, qpr_rd_term(HX[i], G[i], P3[i] + w3b[h]));
      }
    }
    const double fval = wave_sum(fl);
    const double rd_rel = wave_max(m_rd);
    const QprMerit mer = qpr_merit(fval, gap, rd_rel, rp_rel); const double gap_rel = mer.gap_rel, merit = mer.merit;
    fval_s = fval; merit_s = merit;
    const bool res_ok = merit <= P.tol;
#ifdef QP_DEBUG_DUMP
    if (P.dump && P.dump_stage == 5 && b == P.dump_iter && lane == 0 && it < 120) {   // debug: iteration trace of instance `dump_iter`
      double* o_ = P.dump + 16 * it;
      o_[0] = merit; o_[1] = rd_rel; o_[2] = rp_rel; o_[3] = gap_rel; o_[4] = mu; o_[5] = fval; o_[6] = (double)have_saved; o_[7] = saved_merit;
    }
#endif
    if (!(merit < INFINITY)) { flag = have_saved ? 2 : -1; break; }
    const int keep = qpr_keep_rule(merit, rp_rel, gap_rel, P.tol_loose, saved_merit, have_saved);
    if (keep == QPR_KEEP_SAVE) {
      for (int i = lane; i < k.np; i += 64) XS[i] = X[i];
      for (int js = 0; js < JT; ++js) LAMS[js * 64 + lane] = aW3[js * 64 + lane];
      have_saved = 1; saved_merit = merit;
    } else if (keep == QPR_KEEP_REPAIR) {   // only the dual residual is in the way: certificate repair of a copy
      double dgap = 0, m_rd2 = 0, lamfix[2] = {0.0, 0.0};
      for (int h = 0; h < 2; ++h) {
        const int i = lane + 64 * h;
        if (i < n) {
          const int ix = (J + (i >> 6)) * 64 + (i & 63);
          lamfix[h] = qpr_repair(aW3[ix], P3[i], HX[i], G[i], aL[ix], aU[ix], aV[ix], dgap, m_rd2);
        }
      }
      const double merit2 = qpr_repaired_merit(wave_max(m_rd2), rp_rel, gap, wave_sum(dgap), fval);
      if (qpr_beats_saved(merit2, P.tol_loose, saved_merit)) {
        for (int i = lane; i < k.np; i += 64) XS[i] = X[i];
        for (int js = 0; js < J; ++js) LAMS[js * 64 + lane] = aW3[js * 64 + lane];
        for (int h = 0; h < 2; ++h) { const int i = lane + 64 * h; if (i < k.np) LAMS[(J + (i >> 6)) * 64 + (i & 63)] = i < n ? lamfix[h] : 0.0; }
        have_saved = 1; saved_merit = merit2;
      }
      if (have_saved) { flag = 2; break; }
    } else if (keep == QPR_KEEP_RETURN) { flag = 2; break; }
    qpr_progress(merit, best_res, stall);

    // ================= factorise (registers, MFMA) and solve for the affine / centering right-hand sides =================
    for (int h = 0; h < 2; ++h) {
      const int i = lane + 64 * h;
      if (i < k.np) {
        R1[i] = i < n ? -(HX[i] + G[i]) + P1[i] + w1b[h] : 0.0;
        R2[i] = i < n ? P2[i] + w2b[h] : 0.0;
      }
    }
    STAMP(4);
    if (factor_solve2(it)) {
      flag = (res_ok || have_saved) ? 2 : -1;
      // the factorisation broke down (weights ~1e24) on an iterate that is nearly primal feasible and complementary: its working
      // set is usually the right one already, so the refinement gets a try -- it accepts nothing that is not a KKT point of the
      // full QP by a fresh evaluation (flag 4 -> 0 if accepted, else -1)
      if (flag == -1 && P.polish && rp_rel <= QP_BREAKDOWN_TRY_TOL && gap_rel <= QP_BREAKDOWN_TRY_TOL) flag = 4;
      break;
    }
    STAMP(6);
#ifdef QP_DEBUG_DUMP
    if (P.dump && b == 0 && P.dump_stage == 2 && it == P.dump_iter) {
      for (int i = lane; i < n; i += 64) { P.dump[i] = R1[i]; P.dump[n + i] = R2[i]; }
    }
#endif
    if (res_ok) {  // Newton-decrement test in the caller's coordinates
      double dm = 0, xm = 1.0;
      for (int h = 0; h < 2; ++h) {
        const int i = lane + 64 * h;
        if (i < n) { dm = fmax(dm, fabs(R1[i] * EV[i])); xm = fmax(xm, fabs(X[i] * EV[i])); }
      }
      dm = wave_max(dm); xm = wave_max(xm);
      if (dm <= P.tol_x * xm) { flag = 0; break; }
    }
    if (it >= P.max_iter) { flag = have_saved ? 2 : 1; break; }

    // ================= pass 2: va = G dxa, vc = G dxc =================
    {
      const double* vin[2] = {R1, R2}; double* rout[2] = {aVA, aVC};
      pass_Av<T, NB, 2, 1>(k, st, vin, rout, P1);   // fused: P1 = A~' w_cor
    }
    BoundVals bv;   // the variable-bound rows' va = dxa, vc = dxc come straight from R1, R2 (bound_dirs)
    bound_dirs(bv);
    bv.w2[0] = bv.w2[1] = 0.0;
    STAMP(7);
    // ================= row phase 2: affine step length, sigma, corrector weights (one sweep) =================
    // mu_aff(alpha) = [S0 + alpha S1 + alpha^2 S2]/cnt with S0 = sum t z, S1 = sum (t dz + z dt), S2 = sum dt dz
    double a_aff = 1.0, s1 = 0.0, s2 = 0.0;
    double wb[2] = {0.0, 0.0};   // second-order weight of this lane's variable-bound rows (slots J, J + 1): the corrector's right-hand side reads it
    auto row2_body = [&](const Slot& r, int js) {
      double w = 0.0;
      if (qpr_has_lower(r.valid, r.l)) w -= qpr_side_affine(r.tl, r.zl, r.rpl, r.va, a_aff, s1, s2);
      if (qpr_has_upper(r.valid, r.u)) w += qpr_side_affine(r.tu, r.zu, r.rpu, -r.va, a_aff, s1, s2);
      if (js == J) wb[0] = w;       // (A rows: fused in pass 2; an invalid slot has w = 0)
      if (js == J + 1) wb[1] = w;
    };
    sweep(bv, row2_body);
    a_aff = wave_min(a_aff);
    s1 = wave_sum(s1); s2 = wave_sum(s2);
    const QprCenter cen = qpr_centering(gap, cnt, mu, a_aff, s1, s2, P.tol, fval); const double smu = cen.smu, cw = cen.cw;   // (cw = 0: no second-order term, no corrector solve and no pass 3 this iteration)
    WAVE_SYNC();
    STAMP(8);
    if (cw != 0.0) {
    // ================= corrector: P1 = A' w_cor came out of the fused pass 2 =================
    STAMP(9);
    for (int h = 0; h < 2; ++h) {
      const int i = lane + 64 * h;
      if (i < k.np) DX[i] = i < n ? P1[i] + wb[h] : 0.0;
    }
    WAVE_SYNC();
    solve1(DX);
    WAVE_SYNC();
    STAMP(10);
    // ================= pass 4: G dx_cor =================
    {
      const double* vin[1] = {DX}; double* rout[1] = {aW2};  // W2 reused for G dx_cor
      pass_Av<T, NB, 1, 0>(k, st, vin, rout, nullptr);
    }
    STAMP(11);
    } else {   // no corrector this iteration
      for (int i = lane; i < k.np; i += 64) DX[i] = 0.0;
      for (int js = 0; js < J; ++js) aW2[js * 64 + lane] = 0.0;
      WAVE_SYNC();
    }
    // the bound rows' G dx_cor is dx_cor itself: taken here, before DX becomes the full direction
    bound_dirs(bv);
    for (int h = 0; h < 2; ++h) { const int i = lane + 64 * h; bv.w2[h] = i < n ? DX[i] : 0.0; }
    // full direction dx = dxa + smu*dxc + dxcor ; dv likewise
    for (int h = 0; h < 2; ++h) {
      const int i = lane + 64 * h;
      if (i < n) DX[i] = R1[i] + smu * R2[i] + DX[i];
    }
    // ================= row phase 3: step length (Mehrotra heuristic on the blocking pair), update =================
    QprBlock blk = qpr_block_none(); double q1 = 0.0, q2 = 0.0;
    double dvb[2] = {0.0, 0.0};
    auto row3a_body = [&](const Slot& r, int js) {
      const double dv = r.va + smu * r.vc + r.w2;
      if (js < J) aVC[r.ix] = dv;  // keep the full G dx for the update (variable-bound slots: in dvb)
      if (js == J) dvb[0] = dv;
      if (js == J + 1) dvb[1] = dv;
      if (qpr_has_lower(r.valid, r.l)) qpr_side_block(r.tl, r.zl, qpr_side_step(r.tl, r.zl, r.rpl, r.va, dv, smu, cw), blk, q1, q2);
      if (qpr_has_upper(r.valid, r.u)) qpr_side_block(r.tu, r.zu, qpr_side_step(r.tu, r.zu, r.rpu, -r.va, -dv, smu, cw), blk, q1, q2);
    };
    sweep(bv, row3a_body);
    const double amax_w = wave_min(blk.amax);
    double alpha = 1.0;
    if (amax_w < QPR_AMAX_SET) {
      // blocking pair = the one on the lane that attains the minimum (first such lane)
      const unsigned long long msk = __ballot(blk.amax == amax_w);
      const int src = __ffsll((long long)msk) - 1;
      q1 = wave_sum(q1); q2 = wave_sum(q2);
      alpha = qpr_step_length(gap, cnt, amax_w, q1, q2, rl(blk.bp, src), rl(blk.bdp, src), rl(blk.bd, src), rl(blk.bdd, src));
    }
#ifdef QP_DEBUG_DUMP
    if (P.dump && P.dump_stage == 5 && b == P.dump_iter && lane == 0 && it < 120) {
      double* o_ = P.dump + 16 * it;
      o_[8] = a_aff; o_[9] = cen.sigma; o_[10] = alpha; o_[11] = cw; o_[12] = amax_w; o_[13] = (double)stall;
    }
    if (P.dump && b == 0 && P.dump_stage == 4 && it == P.dump_iter) {   // debug: step-length pipeline of this iteration
      double c1 = 0, c2 = 0, c3 = 0, c4 = 0;
      for (int js = 0; js < J; ++js) { const int ix = js * 64 + lane; c1 += aVA[ix]; c2 += aVC[ix]; c3 += aW2[ix]; c4 += aW1[ix]; }   // (A rows: the bound rows' parts never reach these arrays)
      c1 = wave_sum(c1); c2 = wave_sum(c2); c3 = wave_sum(c3); c4 = wave_sum(c4);
      if (lane == 0) {
        double* o_ = P.dump;
        o_[0] = a_aff; o_[1] = cen.mu_aff; o_[2] = cen.sigma; o_[3] = smu; o_[4] = cw; o_[5] = amax_w; o_[6] = alpha; o_[7] = gap; o_[8] = mu;
        o_[9] = c1; o_[10] = c2; o_[11] = c3; o_[12] = c4; o_[13] = s1; o_[14] = s2; o_[15] = q1; o_[16] = q2;
      }
      for (int i = lane; i < n; i += 64) { P.dump[32 + i] = DX[i]; P.dump[32 + n + i] = R1[i]; P.dump[32 + 2 * n + i] = R2[i]; P.dump[32 + 3 * n + i] = P1[i]; }
    }
#endif
    // update, fused with the residual / weight phase of the next iteration
    double xn = 0, zn = 0, s_gap = 0, m_rp = 0;
    auto row3b_body = [&](const Slot& r, int js) {
      if (js >= JT) return;
      const double dv = r.vc;   // full G dx stored by the previous sweep
      double tl = r.tl, zl = r.zl, tu = r.tu, zu = r.zu;
      if (qpr_has_lower(r.valid, r.l)) {
        const QprDir s_ = qpr_side_step(tl, zl, r.rpl, r.va, dv, smu, cw);
        tl += alpha * s_.dt; zl += alpha * s_.dz;
        aTL[r.ix] = tl; aZL[r.ix] = zl;
        zn = fmax(zn, zl);
      }
      if (qpr_has_upper(r.valid, r.u)) {
        const QprDir s_ = qpr_side_step(tu, zu, r.rpu, -r.va, -dv, smu, cw);
        tu += alpha * s_.dt; zu += alpha * s_.dz;
        aTU[r.ix] = tu; aZU[r.ix] = zu;
        zn = fmax(zn, zu);
      }
      const double v = r.v + alpha * dv;
      aV[r.ix] = v;
      row1_body(r.ix, r.valid, r.l, r.u, v, tl, tu, zl, zu, s_gap, m_rp);
    };
    bv.vc[0] = dvb[0]; bv.vc[1] = dvb[1];   // (row3b_body reads the slot's full G dx as its vc)
    sweep(bv, row3b_body);
    for (int h = 0; h < 2; ++h) {
      const int i = lane + 64 * h;
      if (i < n) { X[i] += alpha * DX[i]; xn = fmax(xn, fabs(X[i])); }
    }
    const double rp_prev = rp_rel;
    gap = wave_sum(s_gap);
    rp_rel = wave_max(m_rp);
    xn = wave_max(xn); zn = wave_max(zn);
    WAVE_SYNC();
    STAMP(12);
    if (qpr_exit_rule(xn, zn, rp_prev, fval, stall, have_saved, P.polish, flag)) break;   // divergence -> qpOASES exit codes; stall
  }

  // ---- outputs ----
  // The last iterate (or the best saved one) is returned whatever the exit code: the reference keeps driving on whatever the
  // solver handed back (main.m:163-175).
  const bool v_current = flag == 0 || flag == 4;   // aV still equals G x and fval_s is the objective at x (not so after a restore / an update)
  if (flag == 2) {  // restore the best iterate that met tol_loose
    for (int i = lane; i < k.np; i += 64) X[i] = XS[i];
    for (int js = 0; js < JT; ++js) aW3[js * 64 + lane] = LAMS[js * 64 + lane];
    flag = 0; merit_s = saved_merit;
    WAVE_SYNC();
  } else {
    for (int js = 0; js < JT; ++js) {
      const int ix = js * 64 + lane;
      const bool valid = row_valid(k, js);
      const bool hl = valid && aL[ix] > -INFINITY, hu = valid && aU[ix] < INFINITY;
      aW3[ix] = (hl ? aZL[ix] : 0.0) - (hu ? aZU[ix] : 0.0);
    }
    WAVE_SYNC();
  }
  // ---- active-set refinement: from the interior-point point to the vertex an active-set solver (qpOASES) stops at ----
  // Working set W from the multipliers (side active iff |lambda| exceeds its slack).  Active *bounds* are eliminated
  // exactly: the variable is pinned (huge diagonal, zero right-hand side, value reset after every update) and its
  // multiplier is read off the stationarity residual.  Active *rows* A_W z = b: conjugate gradients on the dual of the
  // augmented problem, operator S = A_W M^-1 A_W' with M = H~ + pin + rho A_W'A_W (resident Cholesky factor).  Its
  // spectrum is clustered at 1/rho plus a few small outliers from nearly dependent active rows (long stretches of the
  // horizon on a track limit): CG removes the outliers in one step each, the fixed-step method of multipliers of round 1
  // could not (rejected 10-20 % of the instances).  One fused stream over A~ per CG step (q = A_W w and A_W'q together),
  // A'p kept by recurrence.  The result is accepted only if a fresh evaluation says it is a KKT point of the full QP;
  // otherwise the interior-point iterate is returned.
#ifdef QP_DEBUG_DUMP
  if (P.dump && P.dump_stage == 5 && b == P.dump_iter && lane == 0) { double* o_ = P.dump + 16 * 120; o_[4] = (double)flag; for (int i_ = 5; i_ < 48; ++i_) o_[i_] = 0.0; }
#endif
  if ((flag == 0 || flag == 4 || flag == 5) && P.polish) {
    const double rho = QPR_RHO, pin = QPR_PIN, rinv = 1.0 / rho;
    double* PA = rowp(k, R_CB1); double* PB = rowp(k, R_RPL); double* PY = rowp(k, R_CC1); double* PS = rowp(k, R_CB2);
    double* PC = rowp(k, R_RPU); double* PP = rowp(k, R_CC2); double* PZ0 = aW2;   // constraint residual c, CG direction p, zeros
    double* ATR = R1; double* ATP = P3;                                               // A_W'r and A_W'p (n-vectors, by recurrence)
    if (!v_current) {
      const double* vin[1] = {X}; double* rout[1] = {aV};
      pass_Av<T, NB, 1, 0>(k, st, vin, rout, nullptr);
      for (int jb = 0; jb < k.JB; ++jb) { const int i = jb * 64 + lane; aV[(J + jb) * 64 + lane] = i < n ? X[i] : 0.0; }
    }
    for (int js = 0; js < JT; ++js) {
      const int ix = js * 64 + lane;
      const double lam = aW3[ix]; const QprSide sd = qpr_working_side(row_valid(k, js), aL[ix], aU[ix], aV[ix], lam);
      PS[ix] = sd.side(); PY[ix] = (sd.active() && js < J) ? lam : 0.0;
    }
    for (int i = lane; i < k.np; i += 64) XS[i] = X[i];   // z of the refinement between attempts (the fall-back copy is no longer needed)
    WAVE_SYNC();
    // up to QP_REFINE_ATTEMPTS attempts: a refinement that ends on a violated inactive row / a multiplier of the wrong sign adds / drops
    // that one row and starts over from the point it reached (single add-drop corrections of an active-set method)
    for (int attempt = 0; attempt < QP_REFINE_ATTEMPTS && flag_polished <= 0; ++attempt) {
    for (int js = 0; js < JT; ++js) {
      const int ix = js * 64 + lane;
      const double sd = PS[ix];
      PA[ix] = sd != 0.0 ? rho : 0.0; PB[ix] = qpr_target(sd, aL[ix], aU[ix]);
      aD[ix] = js < J ? PA[ix] : (sd != 0.0 ? pin : 0.0); aW1[ix] = 0.0; aW2[ix] = 0.0; PC[ix] = 0.0; PP[ix] = 0.0;
    }
    WAVE_SYNC();
    acc_init<T>(k, acc);
    pass_syrk<T, NB>(k, st, acc, P1, P2, P3, MB);
    WAVE_SYNC();
    for (int i = lane; i < k.np; i += 64) { R1[i] = 0.0; R2[i] = 0.0; }
    WAVE_SYNC();
    bool pok = factor_solve2(-1) == 0, retry = false;
    if (!pok) { flag_polished = -5; break; }
    // z: the point reached so far (R1, R2 were the right-hand sides of the factorisation), pinned variables on their bounds
    for (int h = 0; h < 2; ++h) {
      const int i = lane + 64 * h;
      if (i < k.np) { const int ix = (J + (i >> 6)) * 64 + (i & 63); R2[i] = (i < n && PS[ix] != 0.0) ? PB[ix] : XS[i]; }
    }
    WAVE_SYNC();
    const double* cf_eval[3] = {PA, PB, PY};
    const double* cf_cg[3] = {PA, PZ0, PZ0};
    // gradient of the augmented Lagrangian at (z, y): v = A~z, y^ = y - rho c, P1 = A~'y^, P2 = rho A_W'c; then grad = H~z + g - P1
    auto eval_zy = [&]() __attribute__((always_inline)) {
      const double* vin[1] = {R2}; double* rout[2] = {aVA, aVC};
      pass_Av<T, NB, 1, 3>(k, st, vin, rout, P1, P2, cf_eval);
      hx_full(R2);
      WAVE_SYNC();
    };
    if (pok) {
      eval_zy();
      for (int h = 0; h < 2; ++h) {
        const int i = lane + 64 * h;
        if (i < k.np) { const int ix = (J + (i >> 6)) * 64 + (i & 63); DX[i] = (i < n && PS[ix] == 0.0) ? -(HX[i] + G[i] - P1[i]) : 0.0; }
      }
      WAVE_SYNC();
      solve1(DX);
      WAVE_SYNC();
      for (int h = 0; h < 2; ++h) {
        const int i = lane + 64 * h;
        if (i < n) { const int ix = (J + (i >> 6)) * 64 + (i & 63); if (PS[ix] == 0.0) R2[i] += DX[i]; }
      }
      WAVE_SYNC();
      eval_zy();   // c(z): aVA = A~z; P2 = rho A_W'c
      double rs_l = 0.0;
      for (int js = 0; js < J; ++js) {
        const int ix = js * 64 + lane;
        const double cc_ = PA[ix] != 0.0 ? aVA[ix] - PB[ix] : 0.0;
        PC[ix] = cc_; PP[ix] = -cc_; rs_l = fma(cc_, cc_, rs_l);
      }
      double rs = wave_sum(rs_l);
      for (int h = 0; h < 2; ++h) { const int i = lane + 64 * h; if (i < k.np) { ATR[i] = -P2[i] * rinv; ATP[i] = ATR[i]; } }
      WAVE_SYNC();
      for (int cgit = 0; cgit < 12 && pok; ++cgit) {
        double m_eq = 0.0, m_cy = 0.0;
        for (int js = 0; js < J; ++js) {
          const int ix = js * 64 + lane;
          m_eq = fmax(m_eq, fabs(PC[ix]) / fmax(1.0, fabs(PB[ix])));
          m_cy = fmax(m_cy, fabs(PC[ix] * PY[ix]));
        }
        m_eq = wave_max(m_eq); m_cy = wave_max(m_cy);
        if (m_eq <= 1e-11 && m_cy <= 1e-11 * fmax(1.0, fabs(fval_s))) break;
        if (cgit == 11) { pok = false; flag_polished = -6; break; }
        for (int h = 0; h < 2; ++h) {
          const int i = lane + 64 * h;
          if (i < k.np) { const int ix = (J + (i >> 6)) * 64 + (i & 63); DX[i] = (i < n && PS[ix] == 0.0) ? ATP[i] : 0.0; }
        }
        WAVE_SYNC();
        solve1(DX);                                   // w = M^-1 A_W'p
        WAVE_SYNC();
        {
          const double* vin[1] = {DX}; double* rout[2] = {aVA, aVC};
          pass_Av<T, NB, 1, 3>(k, st, vin, rout, P1, P2, cf_cg);   // aVA = A~w; P2 = rho A_W'(A_W w)
        }
        WAVE_SYNC();
        double pq_l = 0.0;
        for (int js = 0; js < J; ++js) { const int ix = js * 64 + lane; if (PA[ix] != 0.0) pq_l = fma(PP[ix], aVA[ix], pq_l); }
        const double pq = wave_sum(pq_l);
        if (!(pq > 0.0) || !(rs > 0.0)) {   // dependent / inconsistent working set: drop the row that carries the stalled direction
          pok = false; flag_polished = -7;
          if (attempt < QP_REFINE_ATTEMPTS - 1) {
            double my = 0.0; int myix = -1;
            for (int js = 0; js < J; ++js) { const int ix = js * 64 + lane; if (PA[ix] != 0.0 && fabs(PP[ix]) > my) { my = fabs(PP[ix]); myix = ix; } }
            const double mx = wave_max(my);
            if (mx > 0.0 && my == mx && myix >= 0) { PS[myix] = 0.0; PY[myix] = 0.0; }
            for (int i = lane; i < k.np; i += 64) XS[i] = R2[i];
            WAVE_SYNC();
            retry = true;
          }
          break;
        }
        const double alpha_ = rs / pq;
        double rsn_l = 0.0;
        for (int js = 0; js < J; ++js) {
          const int ix = js * 64 + lane;
          if (PA[ix] != 0.0) {
            PY[ix] = fma(alpha_, PP[ix], PY[ix]);
            const double cc_ = fma(alpha_, aVA[ix], PC[ix]);
            PC[ix] = cc_; rsn_l = fma(cc_, cc_, rsn_l);
          }
        }
        const double rsn = wave_sum(rsn_l);
        const double beta_ = rsn / rs;
        for (int js = 0; js < J; ++js) { const int ix = js * 64 + lane; if (PA[ix] != 0.0) PP[ix] = fma(beta_, PP[ix], -PC[ix]); }
        for (int h = 0; h < 2; ++h) {
          const int i = lane + 64 * h;
          if (i < k.np) {
            const int ix = (J + (i >> 6)) * 64 + (i & 63);
            if (i < n && PS[ix] == 0.0) R2[i] = fma(alpha_, DX[i], R2[i]);
            ATR[i] = fma(-alpha_ * rinv, P2[i], ATR[i]);
            ATP[i] = fma(beta_, ATP[i], ATR[i]);
          }
        }
        rs = rsn;
        WAVE_SYNC();
        // the masked residual lives in PC; aVA is overwritten by the next A~w, so the test above uses |b| and the last A~w only as scale
      }
    }
    if (pok) {
      // fresh evaluation of the candidate (z, y): everything recomputed from a stream over A~ and H~
      eval_zy();
      double m_rd = 0, m_rp = 0, m_sg = 0, m_cp = 0, fl2 = 0;
      for (int h = 0; h < 2; ++h) {
        const int i = lane + 64 * h;
        if (i < n) {
          const int ix = (J + (i >> 6)) * 64 + (i & 63);
          const double zi = R2[i]; const QprVar o = qpr_kkt_var(HX[i], G[i], P1[i], PS[ix], zi, aL[ix], aU[ix], m_rd, m_sg, m_rp);
          aVC[ix] = o.y;                                            // multiplier of the variable-bound row
          fl2 += 0.5 * zi * HX[i] + G[i] * zi + 0.0 * o.r;   // (0 * r: a non-finite residual must poison the sum -- fmax drops NaN operands)
        }
      }
      for (int js = 0; js < J; ++js) {
        const int ix = js * 64 + lane;
        if (row_valid(k, js)) {
          const double sd = PS[ix];
          qpr_kkt_row(aL[ix], aU[ix], aVA[ix], aVC[ix], sd, sd != 0.0 ? PB[ix] : 0.0, m_rp, m_sg, m_cp, fl2);
        }
      }
      m_rd = wave_max(m_rd); m_rp = wave_max(m_rp); m_sg = wave_max(m_sg); m_cp = wave_max(m_cp);
      const double f2 = wave_sum(fl2);
#ifdef QP_DEBUG_DUMP
      if (P.dump && b < 32 && P.dump_stage == 3 && lane == 0) { double* o_ = P.dump + 64 * b; o_[0] = m_rd; o_[1] = m_rp; o_[2] = m_sg; o_[3] = m_cp; o_[5] = f2; }
      if (P.dump && P.dump_stage == 5 && b == P.dump_iter && lane == 0 && attempt < 8) { double* o_ = P.dump + 16 * 120 + 8 + 5 * attempt; o_[0] = 1.0; o_[1] = m_rd; o_[2] = m_rp; o_[3] = m_sg; o_[4] = m_cp; }
#endif
      const int rej = qpr_accept(m_rd, m_rp, m_sg, m_cp, f2);   // acceptance: stationarity, feasibility, complementarity, multiplier signs
      pok = rej == 0; if (!pok) flag_polished = rej;
      if (!pok && attempt < QP_REFINE_ATTEMPTS - 1 && qpr_correctable(m_rd, m_rp, m_sg)) {
        // single correction of the working set: add the most violated inactive row, else drop the worst wrong-sign row
        double my = 0.0; int myix = -1; double myside = 0.0;
        const bool add = qpr_correct_by_add(m_rp);
        for (int js = 0; js < JT; ++js) {
          const int ix = js * 64 + lane;
          if (!row_valid(k, js)) continue;
          const double l = aL[ix], u = aU[ix], sd = PS[ix];
          const double v = js < J ? aVA[ix] : vec_read(R2 + (js - J) * 64 + lane);
          if (add) {
            if (sd != 0.0) continue;
            const QprAdd a_ = qpr_add_score(l, u, v, js < J);
            if (a_.score > my) { my = a_.score; myix = ix; myside = a_.side(); }
          } else {
            if (sd == 0.0) continue;
            const double sg = qpr_drop_score(sd, aVC[ix], js < J);
            if (sg > my) { my = sg; myix = ix; myside = 0.0; }
          }
        }
        const double mx = wave_max(my);
        if (mx > 0.0 && my == mx && myix >= 0) { PS[myix] = myside; PY[myix] = 0.0; }
        for (int js = 0; js < J; ++js) PY[js * 64 + lane] = PS[js * 64 + lane] != 0.0 ? PY[js * 64 + lane] : 0.0;
        for (int i = lane; i < k.np; i += 64) XS[i] = R2[i];
        WAVE_SYNC();
        continue;   // next attempt from the point reached (R2) with the corrected working set
      }
      if (!pok && attempt < QP_REFINE_ATTEMPTS - 1 && qpr_one_more_step(m_rd)) {   // stationarity above the floor: one more exact step from here
        for (int i = lane; i < k.np; i += 64) XS[i] = R2[i];
        for (int js = 0; js < J; ++js) { const int ix = js * 64 + lane; PY[ix] = PS[ix] != 0.0 ? aVC[ix] : 0.0; }
        WAVE_SYNC();
        continue;
      }
      if (!pok) break;
      if (pok) {
        for (int i = lane; i < k.np; i += 64) X[i] = R2[i];
        for (int js = 0; js < JT; ++js) {
          const int ix = js * 64 + lane;
          aW3[ix] = qpr_clamp_multiplier(PS[ix], aVC[ix]);
        }
        flag_polished = 1 + attempt;
        fval_s = f2; merit_s = qpr_refined_merit(m_rd, m_rp, m_cp, f2);
        flag = 0;
      }
      WAVE_SYNC();
    } else if (!retry) break;
    }   // attempts
  }
  if (flag == 4) flag = -1;   // not certified
  if (flag == 5) flag = 1;
  double* xo = P.x + (size_t)b * d.nu;       // caller's indexing (QpDims::nu: dummy padding variables are skipped)
  for (int i = lane; i < n; i += 64) { const int ui = qp_user_index(d, i); if (ui >= 0) xo[ui] = X[i] * EV[i]; }
  if (P.lambda) {
    double* lo = P.lambda + (size_t)b * (d.nu + k.m);
    for (int jb = 0; jb < k.JB; ++jb) {
      const int i = jb * 64 + lane;
      const int ui = i < n ? qp_user_index(d, i) : -1;
      if (ui >= 0) lo[ui] = aW3[(J + jb) * 64 + lane] / EV[i];
    }
    for (int js = 0; js < J; ++js) {
      const int r = k.perm[js * 64 + lane];   // original row of this sorted position
      if (r >= 0) lo[d.nu + r] = aW3[js * 64 + lane] * Fs[js * 64 + lane];
    }
  }
  if (!(v_current || flag_polished > 0)) {  // objective at the returned point, in the caller's units (H~,g~ scaling is objective preserving)
    WAVE_SYNC();
    hx_full(X);
    WAVE_SYNC();
    double fl = 0;
    for (int h = 0; h < 2; ++h) { const int i = lane + 64 * h; if (i < n) fl += qpr_obj_term(X[i], HX[i], G[i]); }
    fval_s = wave_sum(fl);
  }
  STAMP(13);
  STAMP_OUT;
  st.close();   // every exit of the iteration loop and of the refinement, and the early flags -1 / -2, come through here
#ifdef QP_DEBUG_DUMP
  if (P.dump && P.dump_stage == 5 && b == P.dump_iter && lane == 0) { double* o_ = P.dump + 16 * 120; o_[0] = (double)flag; o_[1] = (double)it; o_[2] = (double)flag_polished; o_[3] = merit_s; }
#endif
  if (lane == 0) {
    P.fval[b] = fval_s;
    P.exitflag[b] = flag;
    P.iter[b] = it;
    if (P.polished) P.polished[b] = flag_polished;
    if (P.kkt) P.kkt[b] = merit_s;
  }
}

#undef aL
#undef aU
#undef aTL
#undef aTU
#undef aZL
#undef aZU
#undef aV
#undef aD
#undef aW1
#undef aW2
#undef aW3
#undef aVA
#undef aVC
#undef aRPL
#undef aRPU
#undef X
#undef G
#undef HX
#undef R1
#undef R2
#undef P1
#undef P2
#undef P3
#undef DX
#undef EV

}  // namespace

template <int T, int NB> static hipError_t launch_solve_TN(const QpParams& P, int batch, hipStream_t st) {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&qp_solve_kernel<T, NB>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.d.lds_solve);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((qp_solve_kernel<T, NB>), dim3(batch), dim3(64), P.d.lds_solve, st, P);
  return hipGetLastError();
}
template <int T> static hipError_t launch_solve_T(const QpParams& P, int batch, hipStream_t st) {
  switch (P.d.NB) {
    case 0: return launch_solve_TN<T, 0>(P, batch, st);
    case 1: return launch_solve_TN<T, 1>(P, batch, st);
    case 4: return launch_solve_TN<T, 4>(P, batch, st);
    default: return hipErrorInvalidValue;
  }
}
