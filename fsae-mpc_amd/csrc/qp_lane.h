// qp_lane.h -- lane-level primitives shared by the two QP solve kernels (qp_solve_kernel.h, qp_wg.hip) and the prep kernel:
// vector typedefs, the wave-level fence, lane broadcasts, DPP / lane-swap reductions.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

typedef double v4d __attribute__((ext_vector_type(4)));
typedef double v2d __attribute__((ext_vector_type(2)));

#define DEVINL __device__ __forceinline__
// Lanes of ONE wave exchange data through LDS (and their own rows of global memory) in program order, and the hardware keeps the
// DS / vector-memory operations of one wave in order, so a workgroup barrier (s_barrier + full s_waitcnt drain) is not needed -- a
// compiler-level fence is (qp_wg.hip says what goes wrong without it).
#define WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)

namespace {

DEVINL double rl(double v, int src) {  // wave-uniform broadcast of lane `src` (src must be wave-uniform)
  int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
  int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
  return __hiloint2double(hi, lo);
}
// Lane move of both halves of a double (VALU speed, no LDS).  ZF = false leaves the destination's old value undefined: no zero is
// written into the destination first (one v_mov per half and move), which is only correct where EVERY lane of the wave is active --
// with bound_ctrl off a disabled source lane leaves `old` in the destination.  All the controls used here (quad_perm,
// row_half_mirror, row_mirror; full row and bank masks) have a valid source lane for every destination lane, so with all 64 lanes
// active `old` is never observable.  ZF = true is the zero-filling form for call sites in (possibly) lane-divergent control flow.
template <int CTRL, bool ZF = false> DEVINL double dpp_f64(double v) {
  int lo, hi;
  if (ZF) {
    lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
  } else {
    lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xf, 0xf, false);
    hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xf, 0xf, false);
  }
  return __hiloint2double(hi, lo);
}
struct OpSum { static DEVINL double f(double a, double b) { return a + b; } };
struct OpMax { static DEVINL double f(double a, double b) { return fmax(a, b); } };
struct OpMin { static DEVINL double f(double a, double b) { return fmin(a, b); } };
// Reduction over the 16 lanes sharing l>>4 (one DPP row) of N independent values; every lane gets the totals.  Pairing: lane^1,
// lane^2, lane <-> 7-lane within 8, lane <-> 15-lane within 16.  Each step is done for all N before the next one, so the N chains
// (move -> add -> move ...) are interleaved in source order and fill each other's DPP hazard slots.
template <class OP, int CTRL, bool ZF, int N> DEVINL void grp16_step(double (&v)[N]) {
  double m[N];
#pragma unroll
  for (int i = 0; i < N; ++i) m[i] = dpp_f64<CTRL, ZF>(v[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = OP::f(v[i], m[i]);
}
template <class OP, bool ZF, int N> DEVINL void grp16_reduce(double (&v)[N]) {
  grp16_step<OP, 0xB1, ZF>(v);    // quad_perm [1,0,3,2]
  grp16_step<OP, 0x4E, ZF>(v);    // quad_perm [2,3,0,1]
  grp16_step<OP, 0x141, ZF>(v);   // row_half_mirror
  grp16_step<OP, 0x140, ZF>(v);   // row_mirror
}
template <int N> DEVINL void grp16_sum(double (&v)[N]) { grp16_reduce<OpSum, false>(v); }
template <int N> DEVINL void grp16_max(double (&v)[N]) { grp16_reduce<OpMax, false>(v); }
template <int N> DEVINL void grp16_min(double (&v)[N]) { grp16_reduce<OpMin, false>(v); }
DEVINL double grp16_sum(double v) { double a[1] = {v}; grp16_reduce<OpSum, false>(a); return a[0]; }
DEVINL double grp16_max(double v) { double a[1] = {v}; grp16_reduce<OpMax, false>(a); return a[0]; }
DEVINL double grp16_min(double v) { double a[1] = {v}; grp16_reduce<OpMin, false>(a); return a[0]; }
// the zero-filling forms (correct with disabled lanes: those contribute a zero)
DEVINL double grp16_sum_zf(double v) { double a[1] = {v}; grp16_reduce<OpSum, true>(a); return a[0]; }
DEVINL double grp16_max_zf(double v) { double a[1] = {v}; grp16_reduce<OpMax, true>(a); return a[0]; }
DEVINL double grp16_min_zf(double v) { double a[1] = {v}; grp16_reduce<OpMin, true>(a); return a[0]; }
// Exchange between the four 16-lane rows of a wave with the gfx950 lane-swap instructions (VALU speed; the ds_bpermute
// round trips of __shfl_xor cost ~100 cycles each and a wave reduction needed twelve of them):
//   v_permlane16_swap a, b : a.row1 <-> b.row0, a.row3 <-> b.row2     v_permlane32_swap a, b : a.rows23 <-> b.rows01
// with a = b = v on entry the two results are (row0,row0,row2,row2) / (row1,row1,row3,row3) resp. (rows01 x2) / (rows23 x2).
struct RowPair { double a, b; };
DEVINL RowPair rows_xor16(double v) {
  const int lo = __double2loint(v), hi = __double2hiint(v);
  const auto l = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
  const auto h = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  return {__hiloint2double(h[0], l[0]), __hiloint2double(h[1], l[1])};
}
DEVINL RowPair rows_xor32(double v) {
  const int lo = __double2loint(v), hi = __double2hiint(v);
  const auto l = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
  const auto h = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
  return {__hiloint2double(h[0], l[0]), __hiloint2double(h[1], l[1])};
}
DEVINL double q_sum(double v) {  // sum over the 4 lane groups (same l&15); every lane gets the total
  RowPair r = rows_xor16(v); v = r.a + r.b;
  r = rows_xor32(v); return r.a + r.b;
}
DEVINL double q_max(double v) { RowPair r = rows_xor16(v); v = fmax(r.a, r.b); r = rows_xor32(v); return fmax(r.a, r.b); }
DEVINL double q_min(double v) { RowPair r = rows_xor16(v); v = fmin(r.a, r.b); r = rows_xor32(v); return fmin(r.a, r.b); }
// whole-wave reductions: DPP within the four 16-lane rows, lane swaps across them (no LDS round trips)
DEVINL double wave_sum(double v) { return q_sum(grp16_sum(v)); }
DEVINL double wave_max(double v) { return q_max(grp16_max(v)); }
DEVINL double wave_min(double v) { return q_min(grp16_min(v)); }
DEVINL double wave_sum_zf(double v) { return q_sum(grp16_sum_zf(v)); }
DEVINL double wave_max_zf(double v) { return q_max(grp16_max_zf(v)); }
DEVINL double wave_min_zf(double v) { return q_min(grp16_min_zf(v)); }
// N independent sums over the four lane groups / over the whole wave, step by step for all N
template <int N> DEVINL void q_sum(double (&v)[N]) {
  RowPair r[N];
#pragma unroll
  for (int i = 0; i < N; ++i) r[i] = rows_xor16(v[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = r[i].a + r[i].b;
#pragma unroll
  for (int i = 0; i < N; ++i) r[i] = rows_xor32(v[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = r[i].a + r[i].b;
}
template <int N> DEVINL void wave_sum(double (&v)[N]) { grp16_sum(v); q_sum(v); }
DEVINL int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }   // a wave-uniform value the compiler could not prove uniform -> SGPR
DEVINL const char* uni(const char* p) {
  const unsigned long long v = reinterpret_cast<unsigned long long>(p);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return reinterpret_cast<const char*>(((unsigned long long)hi << 32) | lo);
}

}  // namespace
