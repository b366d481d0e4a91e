// mpc_params.h -- the vehicle, cost and limit constants of the MPC path as a policy type.  The model functions of
// nlp_model.h, the build (ltv_build.hip), the SQP's evaluation (sqp.hip) and the plant (plant.hip) take the constants from a
// policy object `p`:
//   FixedPar  static constexpr members with the reference's values (ltvmpc_*.m:20-35, f_curv_*.m, f_cart_dyn.m, main.m:84-88): the
//             shipped instantiations; every use folds to the literal it replaced.
//   RtPar     the same names as data members, loaded from a block of FSAEMPC_NPAR doubles (include/fsaempc.h, FSAEMPC_P_*).
// Derived constants (wheelbase, lr / (lr + lf), static axle loads) are members of both, so they are formed once per instance.
// Internal header: anonymous namespace (device code of each translation unit).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "fsaempc.h"

namespace {

#ifndef DEVINL
#define DEVINL __device__ __forceinline__
#endif

struct NoParArgs {};
// Where the kernels of the parameterised entries find their blocks: instance `inst` reads values + inst * stride (stride 0: one
// block shared by the batch); idx (optional) maps the workgroup's index to the instance (the SQP's compacted sub-batches).
struct ParArgs { const double* values; int stride; const int* idx; };

struct FixedPar {
  typedef NoParArgs Args;
  static constexpr bool RT = false;
  static constexpr bool bad = false;
  static constexpr double M = 280, IZ = 200, LF = 0.8672, LR = 0.6183, GRAV = 9.81;
  static constexpr double PB = 12.56, PC = 1.38, PD = 1.60, PE = -0.58;
  static constexpr double QW[3] = {5, 250, 2000}, Q_TERMINAL = 10;          // ltvmpc_*.m:32-33: weights on s, n, mu
  static constexpr double R_ACC = 10, R_STEER = 10;                            // ltvmpc_*.m:34
  static constexpr double R_SOFT0 = 1e8, R_SOFT1 = 1e6, R_SOFT2 = 1e6, R_SOFT3 = 1e4;   // ltvmpc_*.m:35 (kinematic: R_SOFT0 only)
  static constexpr double U_ACC_MAX = 10.0, U_STEER_MAX = 0.4;                 // ltvmpc_*.m:28-29
  static constexpr double DELTA_MAX = 0.4, N_MAX = 0.75, V_MIN = 0, ALAT_MAX = 5.0, SLIP_MAX = 0.1;
  static constexpr double ELL_LONG = 10.0, ELL_LAT = 9.163;                    // dynamic_tyre_linearise_constraints.m:33-39
  static constexpr double PID_KP_V = 16000.0, PID_MAX_F = 2800.0, PID_KP_D = 80.0, PID_MAX_DRATE = 0.8;   // main.m:84-88
  static constexpr double WB = LR + LF, LR_RATIO = LR / (LR + LF);
  static constexpr double FZF = M * GRAV * LR / (LR + LF), FZR = M * GRAV * LF / (LR + LF);
  // violation of v >= V_MIN; V_MIN = 0 here, and -v is the shipped arithmetic (0 - v differs from it in the sign of a zero)
  static DEVINL double below_vmin(double v) { return -v; }
};

struct RtPar {
  typedef ParArgs Args;
  static constexpr bool RT = true;
  double M, IZ, LF, LR, GRAV, PB, PC, PD, PE;
  double QW[3], Q_TERMINAL, R_ACC, R_STEER, R_SOFT0, R_SOFT1, R_SOFT2, R_SOFT3;
  double U_ACC_MAX, U_STEER_MAX, DELTA_MAX, N_MAX, V_MIN, ALAT_MAX, SLIP_MAX, ELL_LONG, ELL_LAT;
  double PID_KP_V, PID_MAX_F, PID_KP_D, PID_MAX_DRATE;
  double WB, LR_RATIO, FZF, FZR;
  bool bad;    // the block cannot describe a car (par_entry_bad): the build writes NaN into g, the plant holds the car
  DEVINL double below_vmin(double v) const { return V_MIN - v; }
};

// Entries that must be > 0 (M, IZ, Q_TERMINAL) and entries that must be >= 0 (weights, slack costs, limits; V_MIN may be any
// finite value, and so may the geometry, the tyre coefficients and the PID gains).  LF + LR > 0 is tested on the sum.
constexpr unsigned PAR_POSITIVE = (1u << FSAEMPC_P_M) | (1u << FSAEMPC_P_IZ) | (1u << FSAEMPC_P_Q_TERMINAL);
constexpr unsigned PAR_NONNEG =
    (1u << FSAEMPC_P_Q_S) | (1u << FSAEMPC_P_Q_N) | (1u << FSAEMPC_P_Q_MU) | (1u << FSAEMPC_P_R_ACC) | (1u << FSAEMPC_P_R_STEER) |
    (1u << FSAEMPC_P_R_SOFT0) | (1u << FSAEMPC_P_R_SOFT1) | (1u << FSAEMPC_P_R_SOFT2) | (1u << FSAEMPC_P_R_SOFT3) |
    (1u << FSAEMPC_P_U_ACC_MAX) | (1u << FSAEMPC_P_U_STEER_MAX) | (1u << FSAEMPC_P_DELTA_MAX) | (1u << FSAEMPC_P_N_MAX) |
    (1u << FSAEMPC_P_ALAT_MAX) | (1u << FSAEMPC_P_SLIP_MAX) | (1u << FSAEMPC_P_ELL_LONG) | (1u << FSAEMPC_P_ELL_LAT) |
    (1u << FSAEMPC_P_PID_MAX_F) | (1u << FSAEMPC_P_PID_MAX_DRATE);
DEVINL bool par_entry_bad(int i, double v) {
  bool b = !(fabs(v) < INFINITY);
  if ((PAR_POSITIVE >> i) & 1u) b = b | !(v > 0);
  if ((PAR_NONNEG >> i) & 1u) b = b | !(v >= 0);
  return b;
}

// PTR: `const double*` (one block per lane: the plant) or a pointer into the constant address space (par_uniform: one block per
// workgroup, read with scalar loads).  The validity test walks all FSAEMPC_NPAR entries; only the ones a kernel uses stay live.
template <class PTR> DEVINL RtPar par_load(PTR c) {
  RtPar p;
  double v[FSAEMPC_NPAR];   // (all loads first, no short-circuit between them: they combine into wide loads)
#pragma unroll
  for (int i = 0; i < FSAEMPC_NPAR; ++i) v[i] = c[i];
  bool bad = false;
#pragma unroll
  for (int i = 0; i < FSAEMPC_NPAR; ++i) bad = bad | par_entry_bad(i, v[i]);
  p.M = v[FSAEMPC_P_M]; p.IZ = v[FSAEMPC_P_IZ]; p.LF = v[FSAEMPC_P_LF]; p.LR = v[FSAEMPC_P_LR]; p.GRAV = v[FSAEMPC_P_GRAV];
  p.PB = v[FSAEMPC_P_PB]; p.PC = v[FSAEMPC_P_PC]; p.PD = v[FSAEMPC_P_PD]; p.PE = v[FSAEMPC_P_PE];
  p.QW[0] = v[FSAEMPC_P_Q_S]; p.QW[1] = v[FSAEMPC_P_Q_N]; p.QW[2] = v[FSAEMPC_P_Q_MU]; p.Q_TERMINAL = v[FSAEMPC_P_Q_TERMINAL];
  p.R_ACC = v[FSAEMPC_P_R_ACC]; p.R_STEER = v[FSAEMPC_P_R_STEER];
  p.R_SOFT0 = v[FSAEMPC_P_R_SOFT0]; p.R_SOFT1 = v[FSAEMPC_P_R_SOFT1]; p.R_SOFT2 = v[FSAEMPC_P_R_SOFT2]; p.R_SOFT3 = v[FSAEMPC_P_R_SOFT3];
  p.U_ACC_MAX = v[FSAEMPC_P_U_ACC_MAX]; p.U_STEER_MAX = v[FSAEMPC_P_U_STEER_MAX]; p.DELTA_MAX = v[FSAEMPC_P_DELTA_MAX];
  p.N_MAX = v[FSAEMPC_P_N_MAX]; p.V_MIN = v[FSAEMPC_P_V_MIN]; p.ALAT_MAX = v[FSAEMPC_P_ALAT_MAX]; p.SLIP_MAX = v[FSAEMPC_P_SLIP_MAX];
  p.ELL_LONG = v[FSAEMPC_P_ELL_LONG]; p.ELL_LAT = v[FSAEMPC_P_ELL_LAT];
  p.PID_KP_V = v[FSAEMPC_P_PID_KP_V]; p.PID_MAX_F = v[FSAEMPC_P_PID_MAX_F]; p.PID_KP_D = v[FSAEMPC_P_PID_KP_D];
  p.PID_MAX_DRATE = v[FSAEMPC_P_PID_MAX_DRATE];
  p.WB = p.LR + p.LF;
  bad = bad | !(p.WB > 0);
  p.LR_RATIO = p.LR / (p.LR + p.LF);
  p.FZF = p.M * p.GRAV * p.LR / (p.LR + p.LF); p.FZR = p.M * p.GRAV * p.LF / (p.LR + p.LF);
  p.bad = bad;
  return p;
}

typedef const __attribute__((address_space(4))) double* par_cptr;
typedef const __attribute__((address_space(4))) int* par_iptr;
// The block of workgroup `wg`, through addresses the compiler can see are uniform and constant for the kernel's duration: the
// loads become scalar loads and the block lives in SGPRs.  (Nothing writes a block or an index list while a kernel that reads it
// runs: the constant address space states exactly that.)
DEVINL RtPar par_uniform(const ParArgs& a, int wg) {
  int inst = wg;
  if (a.idx) inst = ((par_iptr)(a.idx))[wg];
  return par_load((par_cptr)(a.values) + (size_t)inst * (size_t)a.stride);
}

// The same block read again later in a kernel (the pointer is made opaque, so the second read is not merged with the first and the
// values of the first need not stay in registers in between).
DEVINL RtPar par_uniform_again(const ParArgs& a, int wg) {
  int inst = wg;
  if (a.idx) inst = ((par_iptr)(a.idx))[wg];
  par_cptr c = (par_cptr)(a.values) + (size_t)inst * (size_t)a.stride;
  asm volatile("" : "+s"(c));
  return par_load(c);
}
template <class PAR> DEVINL PAR par_get_again(const typename PAR::Args& a, int wg) {
  if constexpr (PAR::RT) return par_uniform_again(a, wg); else return PAR{};
}

// The policy object of a kernel: nothing to load for FixedPar
template <class PAR> DEVINL PAR par_get(const typename PAR::Args& a, int wg) {
  if constexpr (PAR::RT) return par_uniform(a, wg); else return PAR{};
}

}  // namespace
