// qp_rules.h -- the scalar rules of the batched QP solve, written once for both solve kernels (qp_solve_kernel.h: one wavefront per
// QP; qp_wg.hip: one workgroup per QP) and for the host: the arithmetic of one row and the decisions of one iteration of the
// Mehrotra predictor-corrector (OOQP-style step heuristic), and of the active-set refinement behind it.
// What is NOT here: memory, lanes, LDS, the owner layout, QpParams.  Values go in, values come out (several results: a small struct;
// running sums / maxima / minima: by reference, in the order the kernels accumulate them); a kernel that needs only some of the
// results relies on inlining to drop the rest.  `valid` is the caller's row predicate (the one-wavefront kernel: row_valid; the
// workgroup kernel: true -- its padding rows carry infinite bounds); a side of a row exists iff the row is valid and the bound finite.
// The file compiles as plain C++: tests/test_qp_rules_cpu.py builds it with -ffp-contract=off under the sanitizers and compares every
// output with tests/qp_rules_numpy.py, operation for operation.  The order of the floating-point operations is part of the contract.
#pragma once
#include <math.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define QPR_HD __host__ __device__ __forceinline__
#else
#define QPR_HD inline
#endif
#ifndef QP_REFINE_ATTEMPTS
#define QP_REFINE_ATTEMPTS 3
#endif
template <int C> struct IC { static constexpr int value = C; };
// ---- named constants ----
#define QPR_GAMMA_F 0.99       // step length (Mehrotra heuristic on the blocking pair): at least gamma_f of the way to the boundary,
#define QPR_STEP_BACKOFF 0.99999999   // never the whole way
#define QPR_AMAX_UNSET 1e300   // no blocking pair yet; "some pair blocks" is amax < QPR_AMAX_SET
#define QPR_AMAX_SET 1e299
// the second-order term is dropped when the affine step is tiny (it then models nothing and makes the iteration
// cycle on low-speed instances); this also saves the corrector solve and pass 3 for that iteration
#define QPR_CORRECTOR_MIN_STEP 0.05
#define QPR_MU_FLOOR 1e-5      // floor of the centering target sigma * mu: mu_floor = 1e-5 tol max(1, |fval|) / cnt
#define QPR_PROGRESS 0.9       // an iteration counts as progress if the merit falls under 0.9 of the best one so far
// once an iterate met tol_loose, a handful of non-improving iterations means the end game lost its numerical
// footing: return the saved iterate (this also bounds the iteration tail, i.e. the kernel's drain time)
#define QPR_STALL_SAVED 5
#define QPR_STALL_UNSAVED 25
// divergence heuristics -> qpOASES exit codes (qpOASES.m:43-47)
// a diverging iterate is 'unbounded' (-3) only if it is primal feasible and the objective follows it to -infinity;
// with a primal residual it is the signature of an infeasible QP (-2); on a bounded feasible problem (every LTV-MPC QP:
// boxed inputs, slacks with positive linear cost) it is an internal failure (-1)
#define QPR_DIVERGED_X 1e13
#define QPR_DIVERGED_Z 1e15
#define QPR_INFEASIBLE_RP 1e-6
#define QPR_RHO 1e6    // refinement: penalty on the working set's rows and pin of its bounds (M = H~ + pin + rho A_W'A_W)
#define QPR_PIN 1e16
// acceptance: relative stationarity 1e-8 (the 1e8 slack cost of ltvmpc_*.m:35 puts cancellations of 1e8 eps into A'y of
// the active soft rows: the floor of any fp64 evaluation of this residual; qpOASES' own terminationTolerance is
// 5e6 eps = 1.1e-9, qpOASES_options.m:190), feasibility and complementarity 1e-10, multipliers of the right sign
// (round-off level wrong signs are zeroed)
#define QPR_ACCEPT_RD 1e-8
#define QPR_ACCEPT_RP 1e-10
#define QPR_ACCEPT_CP 1e-10
#define QPR_ACCEPT_SG 1e-8
#define QPR_RESTEP_RD 1e-4   // stationarity above the floor but under this: one more exact step from the point reached
// ---- the interior-point iteration ----
// Residuals and barrier weights of one row, everything pass 1 / pass 2 need: primal residuals rpl = v - l - tl, rpu = u - v - tu;
// dl, du = z / t and ccl, ccu = z / t^2 (corrector coefficients CB, CC); barrier weight D, affine rhs weight W1, centering weight
// W2 (times sigma*mu), current multiplier W3 (for the dual residual); the complementarity sum and the relative primal residual
struct QprRow { double rpl, rpu, dl, du, ccl, ccu, D, W1, W2, W3; };
QPR_HD QprRow qpr_row_weights(bool valid, double l, double u, double v, double tl, double tu, double zl, double zu, double& s_gap, double& m_rp) {
  const bool hl = valid && l > -INFINITY, hu = valid && u < INFINITY;
  QprRow o; o.rpl = hl ? v - l - tl : 0.0; o.rpu = hu ? u - v - tu : 0.0;
  o.dl = hl ? zl / tl : 0.0; o.du = hu ? zu / tu : 0.0;
  o.ccl = hl ? o.dl / tl : 0.0; o.ccu = hu ? o.du / tu : 0.0;
  o.D = o.dl + o.du; o.W1 = -o.dl * o.rpl + o.du * o.rpu;
  o.W2 = (hl ? 1.0 / tl : 0.0) - (hu ? 1.0 / tu : 0.0); o.W3 = (hl ? zl : 0.0) - (hu ? zu : 0.0);
  s_gap += (hl ? tl * zl : 0.0) + (hu ? tu * zu : 0.0);
  const double sc = fmax(1.0, fabs(v));
  if (hl) m_rp = fmax(m_rp, fabs(o.rpl) / fmax(sc, fabs(l)));
  if (hu) m_rp = fmax(m_rp, fabs(o.rpu) / fmax(sc, fabs(u)));
  return o;
}
QPR_HD bool qpr_has_lower(bool valid, double l) { return valid && l > -INFINITY; }
QPR_HD bool qpr_has_upper(bool valid, double u) { return valid && u < INFINITY; }
// One existing side (slack t, multiplier z, residual rp) along the affine direction; va is +G dxa for the lower side, -G dxa for the
// upper one.  Ratio test into a_aff, mu_aff(alpha) = [S0 + alpha S1 + alpha^2 S2]/cnt with S0 = sum t z, S1 = sum (t dz + z dt),
// S2 = sum dt dz.  Returns the side's second-order weight dt dz / t (the lower side enters the row's weight with -, the upper with +).
QPR_HD double qpr_side_affine(double t, double z, double rp, double va, double& a_aff, double& s1, double& s2) {
  const double dt = va + rp, dz = -z - (z / t) * dt;
  if (dt < 0) a_aff = fmin(a_aff, -t / dt);  if (dz < 0) a_aff = fmin(a_aff, -z / dz);
  s1 += t * dz + z * dt; s2 += dt * dz;
  return dt * dz / t;
}
// One existing side along the combined direction: dv is +-(G dx) of the full step, smu = sigma mu, cw the corrector switch
struct QprDir { double dt, dz; };
QPR_HD QprDir qpr_side_step(double t, double z, double rp, double va, double dv, double smu, double cw) {
  const double dta = va + rp, dza = -z - (z / t) * dta;
  const double c = smu - cw * dta * dza;
  QprDir o; o.dt = dv + rp; o.dz = -z + c / t - (z / t) * o.dt;
  return o;
}
// Blocking-pair bookkeeping of one side: ratio amax, blocking quantity bp and its step bdp, its partner bd and the partner's step bdd;
// the first pair that attains the smallest ratio keeps the place (a tie does not replace it); q1, q2: S1, S2 of the combined direction
struct QprBlock { double amax, bp, bdp, bd, bdd; };
QPR_HD QprBlock qpr_block_none() { QprBlock b; b.amax = QPR_AMAX_UNSET; b.bp = 0; b.bdp = 0; b.bd = 0; b.bdd = 0; return b; }
QPR_HD void qpr_side_block(double t, double z, const QprDir& d, QprBlock& b, double& q1, double& q2) {
  if (d.dt < 0 && -t / d.dt < b.amax) { b.amax = -t / d.dt; b.bp = t; b.bdp = d.dt; b.bd = z; b.bdd = d.dz; }
  if (d.dz < 0 && -z / d.dz < b.amax) { b.amax = -z / d.dz; b.bp = z; b.bdp = d.dz; b.bd = t; b.bdd = d.dt; }
  q1 += t * d.dz + z * d.dt; q2 += d.dt * d.dz;
}
// mu_aff, sigma with its floor, the corrector switch
struct QprCenter { double mu_aff, sigma, smu, cw; };
QPR_HD QprCenter qpr_centering(double gap, double cnt, double mu, double a_aff, double s1, double s2, double tol, double fval) {
  QprCenter o; o.mu_aff = fmax(0.0, gap + a_aff * (s1 + a_aff * s2)) / cnt;
  double sigma = mu > 0 ? (o.mu_aff / mu) * (o.mu_aff / mu) * (o.mu_aff / mu) : 0.0;
  if (sigma > 1.0) sigma = 1.0;
  const double mu_floor = QPR_MU_FLOOR * tol * fmax(1.0, fabs(fval)) / cnt;
  if (mu > 0 && sigma < mu_floor / mu) sigma = fmin(1.0, mu_floor / mu);
  o.sigma = sigma; o.smu = sigma * mu; o.cw = a_aff >= QPR_CORRECTOR_MIN_STEP ? 1.0 : 0.0;
  return o;
}
// step length from the blocking pair of the whole QP (amax < QPR_AMAX_SET), q1, q2 summed over the QP
QPR_HD double qpr_step_length(double gap, double cnt, double amax, double q1, double q2, double bp, double bdp, double bd, double bdd) {
  const double gamma_f = QPR_GAMMA_F, gamma_a = 1.0 / (1.0 - gamma_f);
  const double mufull = fmax(0.0, gap + amax * (q1 + amax * q2)) / cnt / gamma_a;
  const double a_h = (-bp + mufull / (bd + amax * bdd)) / bdp;
  return fmin(1.0, fmin(QPR_STEP_BACKOFF * amax, fmax(a_h, gamma_f * amax)));
}
// objective and dual residual of one variable; gz = (A~'lambda)_i, rows and bound together
QPR_HD double qpr_obj_term(double x, double hx, double g) { return 0.5 * x * hx + g * x; }
QPR_HD double qpr_rd_scale(double hx, double g, double gz) { return fmax(1.0, fmax(fabs(g), fmax(fabs(hx), fabs(gz)))); }
QPR_HD double qpr_rd_term(double hx, double g, double gz) { return fabs(hx + g - gz) / qpr_rd_scale(hx, g, gz); }
// (fmax drops NaN operands: an iterate with NaN in it -- a step along a direction from a broken-down factorisation, 0 * NaN --
//  would read as merit 0.  Its objective is NaN, and so must the merit be: the best saved iterate is returned then.)
struct QprMerit { double gap_rel, merit; };
QPR_HD QprMerit qpr_merit(double fval, double gap, double rd_rel, double rp_rel) {
  QprMerit o; o.gap_rel = gap / fmax(1.0, fabs(fval));
  o.merit = (fabs(fval) < INFINITY && fabs(o.gap_rel) < INFINITY) ? fmax(rd_rel, fmax(rp_rel, o.gap_rel)) : INFINITY;
  return o;
}
// What an iterate with a finite merit means for the fall-back copy.  SAVE: it meets tol_loose and beats the saved one.  REPAIR: only
// the dual residual is in the way (the Newton steps lose accuracy once z/t passes ~1e19 and r_d creeps up): repair the certificate of
// a *copy* of the iterate (qpr_repair); the copy qualifies as fall-back if its complementarity stays within tol_loose
// (qpr_repaired_merit).  RETURN: past tol_loose again with a saved iterate: return that one (flag 2).
QPR_HD bool qpr_beats_saved(double merit, double tol_loose, double saved_merit) { return merit <= tol_loose && merit < saved_merit; }
enum { QPR_KEEP_NONE = 0, QPR_KEEP_SAVE, QPR_KEEP_REPAIR, QPR_KEEP_RETURN };
QPR_HD int qpr_keep_rule(double merit, double rp_rel, double gap_rel, double tol_loose, double saved_merit, int have_saved) {
  if (qpr_beats_saved(merit, tol_loose, saved_merit)) return QPR_KEEP_SAVE;
  else if (merit > tol_loose && rp_rel <= tol_loose && gap_rel <= tol_loose) return QPR_KEEP_REPAIR;
  else if (have_saved && merit > tol_loose) return QPR_KEEP_RETURN;
  return QPR_KEEP_NONE;
}
// Certificate repair of one variable: r_d moves into the bound multiplier where a finite bound of the right sign exists (returns the
// repaired multiplier, the complementarity it costs goes to dgap); elsewhere the multiplier stays and the residual counts (m_rd2)
QPR_HD double qpr_repair(double lam, double p3, double hx, double g, double l, double u, double v, double& dgap, double& m_rd2) {
  const double gz = p3 + lam, r = hx + g - gz;
  const double lam2 = lam + r; const bool ok = lam2 >= 0 ? l > -INFINITY : u < INFINITY;
  if (ok) { dgap += fabs(r) * fmax(0.0, lam2 >= 0 ? v - l : u - v); return lam2; }
  m_rd2 = fmax(m_rd2, fabs(r) / qpr_rd_scale(hx, g, gz));
  return lam;
}
QPR_HD double qpr_repaired_merit(double rd2, double rp_rel, double gap, double dgap, double fval) { return fmax(rd2, fmax(rp_rel, (gap + dgap) / fmax(1.0, fabs(fval)))); }
QPR_HD void qpr_progress(double merit, double& best_res, int& stall) { if (merit < QPR_PROGRESS * best_res) { best_res = merit; stall = 0; } else ++stall; }
// End of an iteration: true if the loop ends here, with the exit code in flag (5: stalled, the refinement may still certify, else 1)
QPR_HD bool qpr_exit_rule(double xn, double zn, double rp_prev, double fval, int stall, int have_saved, int polish, int& flag) {
  if (xn > QPR_DIVERGED_X) { flag = rp_prev > QPR_INFEASIBLE_RP ? -2 : (fval < -QPR_DIVERGED_X ? -3 : -1); return true; }
  if (zn > QPR_DIVERGED_Z && rp_prev > QPR_INFEASIBLE_RP) { flag = -2; return true; }
  if (stall > (have_saved ? QPR_STALL_SAVED : QPR_STALL_UNSAVED)) { flag = have_saved ? 2 : (rp_prev > QPR_INFEASIBLE_RP ? -2 : (polish ? 5 : 1)); return true; }
  return false;
}
// ---- the active-set refinement ----
// working set from the multipliers: a side is active iff its multiplier has the side's sign and exceeds the side's slack
struct QprSide {
  bool lo, up;
  QPR_HD double side() const { return lo ? 1.0 : (up ? -1.0 : 0.0); }
  QPR_HD bool active() const { return lo || up; }
};
QPR_HD QprSide qpr_working_side(bool valid, double l, double u, double v, double lam) {
  QprSide o; o.lo = valid && l > -INFINITY && lam > 0 && lam > fabs(v - l);
  o.up = valid && u < INFINITY && lam < 0 && -lam > fabs(u - v);
  return o;
}
QPR_HD double qpr_target(double sd, double l, double u) { return sd > 0 ? l : (sd < 0 ? u : 0.0); }
// Fresh evaluation, one variable: r = (H~z + g - A~'y)_i must vanish on a free variable (m_rd) and is the bound multiplier of a
// pinned one (sign: m_sg); zi against its bounds (m_rp).  Returns r and the multiplier of the variable-bound row.  (The objective
// term 0.5 zi hx + g zi + 0 r stays with each kernel: inside this function the compiler contracts it into other FMAs than in place,
// and the refined fval and kkt change in the last bit.)
struct QprVar { double r, y; };
QPR_HD QprVar qpr_kkt_var(double hx, double g, double p1, double sd, double zi, double l, double u, double& m_rd, double& m_sg, double& m_rp) {
  const double r = hx + g - p1, sc = qpr_rd_scale(hx, g, p1);
  if (sd == 0.0) m_rd = fmax(m_rd, fabs(r) / sc);
  else m_sg = fmax(m_sg, (sd > 0 ? -r : r) / sc);
  double viol = 0.0;
  if (l > -INFINITY && zi < l) viol = l - zi;
  if (u < INFINITY && zi > u) viol = fmax(viol, zi - u);
  m_rp = fmax(m_rp, viol / fmax(1.0, fabs(zi)));
  QprVar o; o.r = r; o.y = sd != 0.0 ? r : 0.0; return o;
}
// Fresh evaluation, one valid A row: value v = (A~z)_j, multiplier y, side sd, target tgt (read only on the working set)
QPR_HD void qpr_kkt_row(double l, double u, double v, double y, double sd, double tgt, double& m_rp, double& m_sg, double& m_cp, double& fl2) {
  double sc = fmax(1.0, fabs(v)), viol = 0.0;
  if (l > -INFINITY) sc = fmax(sc, fabs(l));  if (u < INFINITY) sc = fmax(sc, fabs(u));
  if (sd != 0.0) { viol = fabs(v - tgt); m_cp = fmax(m_cp, fabs(y) * viol); }
  if (l > -INFINITY && v < l) viol = fmax(viol, l - v);
  if (u < INFINITY && v > u) viol = fmax(viol, v - u);
  m_rp = fmax(m_rp, viol / sc);
  m_sg = fmax(m_sg, (sd > 0 ? -y : (sd < 0 ? y : 0.0)) / fmax(1.0, fabs(y)));
  fl2 += 0.0 * (v + y);
}
// Acceptance of the candidate: 0, or the flag_polished code of the first test it fails (-5 not finite, -1 stationarity,
// -2 feasibility, -4 multiplier sign, -3 complementarity)
QPR_HD int qpr_accept(double m_rd, double m_rp, double m_sg, double m_cp, double f2) {
  const bool pok = m_rd <= QPR_ACCEPT_RD && m_rp <= QPR_ACCEPT_RP && m_cp <= QPR_ACCEPT_CP * fmax(1.0, fabs(f2)) && m_sg <= QPR_ACCEPT_SG &&
                   fabs(f2) < INFINITY;   // (f2 is NaN if anything in the candidate is not finite)
  if (pok) return 0;
  return !(fabs(f2) < INFINITY) ? -5 : (!(m_rd <= QPR_ACCEPT_RD) ? -1 : (!(m_rp <= QPR_ACCEPT_RP) ? -2 : (!(m_sg <= QPR_ACCEPT_SG) ? -4 : -3)));
}
// a rejected candidate that is stationary: single correction of the working set (add the most violated inactive row if the point
// is infeasible, else drop the worst wrong-sign row); stationarity above the floor: one more exact step from the point reached
QPR_HD bool qpr_correctable(double m_rd, double m_rp, double m_sg) { return m_rd <= QPR_ACCEPT_RD && (m_rp > QPR_ACCEPT_RP || m_sg > QPR_ACCEPT_SG); }
QPR_HD bool qpr_correct_by_add(double m_rp) { return m_rp > QPR_ACCEPT_RP; }
QPR_HD bool qpr_one_more_step(double m_rd) { return !(m_rd <= QPR_ACCEPT_RD) && m_rd <= QPR_RESTEP_RD; }
QPR_HD double qpr_refined_merit(double m_rd, double m_rp, double m_cp, double f2) { return fmax(m_rd, fmax(m_rp, m_cp / fmax(1.0, fabs(f2)))); }
// candidate scores of the correction; a_row: an A row (scaled by its bounds / multiplier), else a variable-bound row
struct QprAdd {
  double score; bool lower;   // relative violation of the worse side; that side is the lower one
  QPR_HD double side() const { return lower ? 1.0 : -1.0; }
};
QPR_HD QprAdd qpr_add_score(double l, double u, double v, bool a_row) {
  double sc = fmax(1.0, fabs(v));
  if (a_row) { if (l > -INFINITY) sc = fmax(sc, fabs(l)); if (u < INFINITY) sc = fmax(sc, fabs(u)); }
  const double vl = l > -INFINITY ? (l - v) / sc : -1.0, vu = u < INFINITY ? (v - u) / sc : -1.0;
  QprAdd o; o.score = fmax(vl, vu); o.lower = vl >= vu; return o;
}
QPR_HD double qpr_drop_score(double sd, double y, bool a_row) { const double sc = a_row ? fmax(1.0, fabs(y)) : 1.0; return (sd > 0 ? -y : y) / sc; }
// multiplier of an accepted point: of its side's sign, or zero
QPR_HD double qpr_clamp_multiplier(double sd, double y) { return sd > 0 ? fmax(y, 0.0) : (sd < 0 ? fmin(y, 0.0) : 0.0); }
