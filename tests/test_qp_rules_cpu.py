"""CPU test of csrc/qp_rules.h, the scalar rules both QP solve kernels call: a stand-alone host program around the header, built with
-ffp-contract=off under the address and undefined-behaviour sanitizers, reads the cases below from a file and writes every rule's
outputs; they must equal the numpy restatement (tests/qp_rules_numpy.py) bit for bit -- with contraction off the same expressions
give the same doubles.  The cases are chosen to take every branch of every rule."""
import os
import shutil
import struct
import subprocess

import numpy as np

import qp_rules_numpy as qr

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
inf, nan = float("inf"), float("nan")
UP = lambda v: float(np.nextafter(v, inf))      # the next double above / below a threshold
DN = lambda v: float(np.nextafter(v, -inf))

CASES = [
    # ROW valid l u v tl tu zl zu s_gap m_rp: lower only, upper only, both (m_rp kept / replaced), neither, invalid, |bound| as the scale
    ("ROW", 1, -1.0, inf, 0.3, 1.2, 1.0, 3.0, 7.0, 0.5, 0.0), ("ROW", 1, -inf, 2.0, 0.3, 1.0, 1.6, 7.0, 2.5, 0.5, 0.01),
    ("ROW", 1, -1.0, 2.0, 0.3, 1.25, 1.75, 3.0, 2.5, 1.0, 10.0), ("ROW", 1, -1.0, 2.0, 0.3, 1.25, 1.75, 3.0, 2.5, 1.0, 0.0),
    ("ROW", 1, -inf, inf, 0.3, 1.0, 1.0, 0.0, 0.0, 0.25, 0.125), ("ROW", 0, -1.0, 2.0, 0.3, 1.25, 1.75, 3.0, 2.5, 0.25, 0.125),
    ("ROW", 1, -50.0, 70.0, 0.3, 49.0, 71.0, 1e-3, 1e4, 0.0, 0.0), ("ROW", 1, -1.0, 2.0, 123.0, 1e-9, 1e-7, 1e10, 1e12, 0.0, 0.0),
    # AFF t z rp va a_aff s1 s2: dt < 0 alone, dz < 0 alone, both, neither ratio shorter than a_aff; the upper side passes -va
    ("AFF", 1.0, 2.0, 0.1, -1.6, 1.0, 0.0, 0.0), ("AFF", 1.0, 2.0, 0.1, 0.4, 1.0, 0.5, -0.25), ("AFF", 1.0, 2.0, 0.1, -0.6, 5.0, 0.0, 0.0),
    ("AFF", 1.0, 2.0, 0.1, -0.6, 0.25, 1.0, 1.0), ("AFF", 3.0, 0.5, -0.2, -(-0.7), 1.0, 0.0, 0.0), ("AFF", 3.0, 0.5, -0.2, -(4.7), 1.0, 0.0, 0.0),
    # STEP t z rp va dv smu cw: corrector on / off, both signs of the directions
    ("STEP", 1.0, 2.0, 0.1, -0.6, -0.4, 0.05, 1.0), ("STEP", 1.0, 2.0, 0.1, -0.6, -0.4, 0.05, 0.0), ("STEP", 3.0, 0.5, -0.2, 0.7, 0.9, 1e-3, 1.0),
    ("STEP", 1e-8, 1e8, 1e-9, -3e-9, -2e-9, 1e-4, 1.0),
    # BLK t z dt dz amax bp bdp bd bdd q1 q2: amax unset, dt blocks, dz blocks, dz shorter than dt, a tie keeps the first, nothing blocks
    ("BLK", 1.0, 2.0, -2.0, 1.0, 1e300, 0, 0, 0, 0, 0.0, 0.0), ("BLK", 1.0, 2.0, 0.5, -3.0, 1e300, 0, 0, 0, 0, 0.5, 0.25),
    ("BLK", 1.0, 2.0, -0.5, -8.0, 1e300, 0, 0, 0, 0, 0.0, 0.0), ("BLK", 1.0, 2.0, -2.0, 1.0, 0.5, 9.0, 8.0, 7.0, 6.0, 1.0, 1.0),
    ("BLK", 1.0, 2.0, -2.0, -4.0, 0.75, 9.0, 8.0, 7.0, 6.0, 1.0, 1.0), ("BLK", 1.0, 2.0, 0.5, 0.25, 1e300, 0, 0, 0, 0, 0.0, 0.0),
    ("BLK", 1.0, 2.0, -2.0, -4.0, 0.25, 9.0, 8.0, 7.0, 6.0, 1.0, 1.0),
    # CEN gap cnt mu a_aff s1 s2 tol fval: plain, mu = 0, sigma clipped at 1, lifted to the floor, floor / mu > 1, negative mu_aff
    # clipped at 0, a_aff on both sides of the corrector switch
    ("CEN", 10.0, 4.0, 2.5, 0.5, -8.0, 1.0, 1e-9, 3.0), ("CEN", 0.0, 4.0, 0.0, 0.5, -8.0, 1.0, 1e-9, 3.0), ("CEN", 10.0, 4.0, 2.5, 0.5, 8.0, 1.0, 1e-9, 3.0),
    ("CEN", 1e-3, 4.0, 2.5e-4, 1.0, -1e-3, 0.0, 1e-2, 1e3), ("CEN", 4e-6, 4.0, 1e-6, 1.0, -4e-6, 0.0, 1e-2, 1e3), ("CEN", 1.0, 4.0, 0.25, 1.0, -3.0, 0.5, 1e-9, -7.0),
    ("CEN", 10.0, 4.0, 2.5, DN(0.05), -8.0, 1.0, 1e-9, 3.0), ("CEN", 10.0, 4.0, 2.5, 0.05, -8.0, 1.0, 1e-9, 3.0),
    # LEN gap cnt amax q1 q2 bp bdp bd bdd: a_h above the back-off, under gamma_f amax, in between, a long step capped at 1
    ("LEN", 10.0, 4.0, 0.5, -8.0, 1.0, 1.0, -2.0, 2.0, 1.0), ("LEN", 10.0, 4.0, 0.5, -30.0, 1.0, 1.0, -2.0, 2.0, 1.0), ("LEN", 1.0, 4.0, 0.5, -1.0, 1.0, 1.0, -2.0, 1e-3, 1e-3),
    ("LEN", 10.0, 4.0, 3.5, -1.0, 0.1, 7.0, -2.0, 2.0, 1.0),
    # KKT x hx g gz, MER fval gap rd rp (a non-finite objective: merit INFINITY, not 0)
    ("KKT", 0.5, -3.0, 2.0, 0.25), ("KKT", -7.0, 1e9, -1e9, 12.0), ("KKT", 1.0, nan, 2.0, 0.25),
    ("MER", 3.0, 1e-7, 1e-9, 1e-8), ("MER", -1e4, 1e-3, 1e-5, 1e-9), ("MER", nan, 1e-7, 1e-9, 1e-8), ("MER", inf, 1e-7, 1e-9, 1e-8), ("MER", 3.0, inf, 1e-9, 1e-8),
    ("MER", 3.0, nan, 1e-9, 1e-8),
    # KEEP merit rp gap_rel tol_loose saved have_saved: save, not better than the saved one, repair, return the saved one, go on
    ("KEEP", 1e-7, 1e-8, 1e-8, 1e-6, inf, 0), ("KEEP", 1e-7, 1e-8, 1e-8, 1e-6, 1e-7, 1), ("KEEP", 1e-4, 1e-8, 1e-8, 1e-6, inf, 0), ("KEEP", 1e-4, 1e-8, 1e-8, 1e-6, 1e-7, 1),
    ("KEEP", 1e-4, 1e-3, 1e-8, 1e-6, 1e-7, 1), ("KEEP", 1e-4, 1e-3, 1e-8, 1e-6, inf, 0), ("KEEP", 1e-6, 1e-8, 1e-8, 1e-6, inf, 0), ("KEEP", 1e-4, 1e-8, 1e-3, 1e-6, inf, 0),
    # REP lam p3 hx g l u v dgap m_rd2: lam2 >= 0 with / without a finite lower bound, lam2 < 0 with / without a finite upper bound,
    # a bound already violated (no complementarity cost)
    ("REP", 0.5, 1.0, 3.0, -1.0, -2.0, inf, 0.5, 0.125, 0.0), ("REP", 0.5, 1.0, 3.0, -1.0, -inf, 4.0, 0.5, 0.125, 1e-3), ("REP", 0.5, 1.0, -3.0, -1.0, -2.0, 4.0, 0.5, 0.125, 0.0),
    ("REP", 0.5, 1.0, -3.0, -1.0, -2.0, inf, 0.5, 0.125, 5.0), ("REP", 0.5, 1.0, 3.0, -1.0, 2.0, inf, 0.5, 0.125, 0.0),
    ("RMER", 1e-9, 1e-8, 1e-6, 2e-6, -40.0), ("RMER", 1e-3, 1e-8, 1e-6, 2e-6, 0.5),
    # PROG merit best_res stall
    ("PROG", 1e-3, inf, 4), ("PROG", 0.89, 1.0, 4), ("PROG", 0.9, 1.0, 4), ("PROG", 0.95, 1.0, 0),
    # EXIT xn zn rp_prev fval stall have_saved polish flag: each threshold from both sides
    ("EXIT", 1e13, 1.0, 1e-5, 0.0, 0, 0, 1, 1), ("EXIT", UP(1e13), 1.0, 1e-5, 0.0, 0, 0, 1, 1), ("EXIT", UP(1e13), 1.0, 1e-6, -2e13, 0, 0, 1, 1),
    ("EXIT", UP(1e13), 1.0, 1e-7, -1e13, 0, 0, 1, 1), ("EXIT", 2e13, 1.0, UP(1e-6), -2e13, 0, 0, 1, 1), ("EXIT", 1.0, 1e15, 1e-5, 0.0, 0, 0, 1, 1),
    ("EXIT", 1.0, UP(1e15), 1e-5, 0.0, 0, 0, 1, 1), ("EXIT", 1.0, 2e15, 1e-6, 0.0, 0, 0, 1, 1), ("EXIT", 1.0, 1.0, 1e-5, 0.0, 5, 1, 1, 1), ("EXIT", 1.0, 1.0, 1e-5, 0.0, 6, 1, 1, 1),
    ("EXIT", 1.0, 1.0, 1e-7, 0.0, 25, 0, 1, 1), ("EXIT", 1.0, 1.0, 1e-7, 0.0, 26, 0, 1, 1), ("EXIT", 1.0, 1.0, 1e-7, 0.0, 26, 0, 0, 1), ("EXIT", 1.0, 1.0, 1e-5, 0.0, 26, 0, 1, 1),
    ("EXIT", 1.0, 1.0, 1e-7, 0.0, 6, 0, 1, 1),
    # SIDE valid l u v lam, TGT sd l u
    ("SIDE", 1, -1.0, 2.0, -0.99, 0.5), ("SIDE", 1, -1.0, 2.0, 0.0, 0.5), ("SIDE", 1, -1.0, 2.0, 1.99, -0.5), ("SIDE", 1, -1.0, 2.0, 1.0, -0.5), ("SIDE", 0, -1.0, 2.0, -0.99, 0.5),
    ("SIDE", 1, -1.0, 2.0, -1.0, 0.0), ("SIDE", 1, -inf, 2.0, 0.0, 0.5), ("SIDE", 1, -1.0, inf, 0.0, -0.5), ("SIDE", 1, -1.0, 2.0, 0.0, nan),
    ("TGT", 1.0, -1.0, 2.0), ("TGT", -1.0, -1.0, 2.0), ("TGT", 0.0, -1.0, 2.0),
    # KVAR hx g p1 sd zi l u m_rd m_sg m_rp: free, pinned below / above, bound violations, a non-finite residual
    ("KVAR", 3.0, -1.0, 2.0 - 1e-9, 0.0, 0.5, -1.0, 2.0, 0.0, 0.0, 0.0), ("KVAR", 3.0, -1.0, 1.0, 1.0, -1.0, -1.0, 2.0, 1e-9, 0.0, 0.0),
    ("KVAR", 3.0, -1.0, 1.0, -1.0, 2.0, -1.0, 2.0, 1e-9, 0.0, 0.0), ("KVAR", 3.0, -1.0, 5.0, 1.0, -1.0, -1.0, 2.0, 1e-9, 2.0, 0.0),
    ("KVAR", 3.0, -1.0, 2.0, 0.0, -1.5, -1.0, 2.0, 0.0, 0.0, 0.0), ("KVAR", 3.0, -1.0, 2.0, 0.0, 2.5, -1.0, 2.0, 0.0, 0.0, 1.0),
    ("KVAR", 3.0, -1.0, 2.0, 0.0, 2.5, -inf, inf, 0.0, 0.0, 0.0), ("KVAR", inf, -1.0, inf, 0.0, 0.5, -1.0, 2.0, 0.0, 0.0, 0.0),
    # KROW l u v y sd tgt m_rp m_sg m_cp fl2: inactive inside / outside its bounds, active on / off its target, one-sided rows, wrong sign
    ("KROW", -1.0, 2.0, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.5), ("KROW", -1.0, 2.0, -1.5, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.5), ("KROW", -1.0, 2.0, 2.5, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.5),
    ("KROW", -1.0, 2.0, -1.0 + 1e-12, 3.0, 1.0, -1.0, 0.0, 0.0, 0.0, 1.5), ("KROW", -1.0, 2.0, 2.0 - 1e-12, 3.0, -1.0, 2.0, 0.0, 0.0, 0.0, 1.5),
    ("KROW", -1.0, 2.0, -1.0, -3.0, 1.0, -1.0, 0.0, 0.0, 0.0, 1.5), ("KROW", -70.0, inf, -71.0, 0.0, 0.0, 0.0, 0.5, 0.0, 0.0, 1.5), ("KROW", -inf, 90.0, 91.0, 0.5, -1.0, 90.0, 0.0, 0.0, 1.0, 1.5),
    ("KROW", -1.0, 2.0, 0.5, nan, 1.0, -1.0, 0.0, 0.0, 0.0, 1.5),
    # ACC m_rd m_rp m_sg m_cp f2: each of the four thresholds from both sides, f2 = NaN / Inf, the one-more-step window; codes 0, -1 .. -5
    ("ACC", 1e-8, 1e-10, 1e-8, 1e-10, 0.5), ("ACC", UP(1e-8), 1e-10, 1e-8, 1e-10, 0.5), ("ACC", 1e-8, UP(1e-10), 1e-8, 1e-10, 0.5), ("ACC", 1e-8, 1e-10, UP(1e-8), 1e-10, 0.5),
    ("ACC", 1e-8, 1e-10, 1e-8, UP(1e-10), 0.5), ("ACC", 1e-8, 1e-10, 1e-8, 1e-10 * 100.0, -100.0), ("ACC", 1e-8, 1e-10, 1e-8, UP(1e-10 * 100.0), -100.0),
    ("ACC", 1e-9, 1e-11, 1e-9, 1e-11, nan), ("ACC", 1e-9, 1e-11, 1e-9, 1e-11, inf), ("ACC", 1e-4, 1e-11, 1e-9, 1e-11, 0.5), ("ACC", UP(1e-4), 1e-11, 1e-9, 1e-11, 0.5),
    ("ACC", 1e-9, 1e-3, 1e-3, 1e-3, 0.5), ("ACC", nan, 1e-11, 1e-9, 1e-11, 0.5),
    # ADD l u v a_row, DROP sd y a_row: an add and a drop candidate on an A row and on a bound row; CLAMP sd y
    ("ADD", -1.0, 2.0, -1.5, 1), ("ADD", -1.0, 2.0, 2.5, 1), ("ADD", -50.0, 70.0, 75.0, 1), ("ADD", -50.0, 70.0, 75.0, 0), ("ADD", -inf, 2.0, 2.5, 1), ("ADD", -1.0, inf, -3.0, 0),
    ("ADD", -inf, inf, 0.5, 1), ("ADD", -1.0, 1.0, 0.0, 1),
    ("DROP", 1.0, -3.0, 1), ("DROP", -1.0, 3.0, 1), ("DROP", 1.0, -3.0, 0), ("DROP", -1.0, 0.25, 0), ("DROP", 1.0, 0.25, 1),
    ("CLAMP", 1.0, 0.5), ("CLAMP", 1.0, -1e-13), ("CLAMP", -1.0, -0.5), ("CLAMP", -1.0, 1e-13), ("CLAMP", 0.0, 0.5),
]

HOST_MAIN = r"""
// Stand-alone host program around csrc/qp_rules.h: one case per line of the input file (a tag and its arguments), one line of outputs
// per case, doubles as hexadecimal floating point.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "qp_rules.h"
static void put(const char* tag, const double* o, int n) { printf("%s", tag); for (int i = 0; i < n; ++i) printf(" %a", o[i]); printf("\n"); }
int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 3;
  static_assert(IC<7>::value == 7 && QP_REFINE_ATTEMPTS == 3, "constants of the header");
  printf("CONST %a %a %a %a %a %a %a %a %a %a %a %a %a %a %a %a\n", QPR_GAMMA_F, QPR_STEP_BACKOFF, QPR_AMAX_UNSET, QPR_AMAX_SET, QPR_CORRECTOR_MIN_STEP,
         QPR_MU_FLOOR, QPR_PROGRESS, (double)QPR_STALL_SAVED, (double)QPR_STALL_UNSAVED, QPR_DIVERGED_X, QPR_DIVERGED_Z, QPR_INFEASIBLE_RP, QPR_RHO, QPR_PIN,
         QPR_ACCEPT_RD, QPR_RESTEP_RD);
  char line[1024];
  while (fgets(line, sizeof line, f)) {
    char tag[16]; int used = 0, n = 0;
    if (sscanf(line, "%15s%n", tag, &used) != 1) continue;
    double* a = (double*)malloc(12 * sizeof(double));   // exact size on the heap: the sanitizers see any step outside
    for (char* p = line + used; n < 12; ++n) { char* e; a[n] = strtod(p, &e); if (e == p) break; p = e; }
    double o[12];
    if (!strcmp(tag, "ROW")) {
      double sg = a[8], mr = a[9];
      const QprRow r = qpr_row_weights(a[0] != 0, a[1], a[2], a[3], a[4], a[5], a[6], a[7], sg, mr);
      const double v[12] = {r.rpl, r.rpu, r.dl, r.du, r.ccl, r.ccu, r.D, r.W1, r.W2, r.W3, sg, mr}; put(tag, v, 12);
    } else if (!strcmp(tag, "AFF")) {
      o[1] = a[4]; o[2] = a[5]; o[3] = a[6]; o[0] = qpr_side_affine(a[0], a[1], a[2], a[3], o[1], o[2], o[3]); put(tag, o, 4);
    } else if (!strcmp(tag, "STEP")) {
      const QprDir d = qpr_side_step(a[0], a[1], a[2], a[3], a[4], a[5], a[6]); o[0] = d.dt; o[1] = d.dz; put(tag, o, 2);
    } else if (!strcmp(tag, "BLK")) {
      QprBlock b = qpr_block_none();
      if (a[4] != b.amax || b.bp != 0 || b.bdp != 0 || b.bd != 0 || b.bdd != 0) { b.amax = a[4]; b.bp = a[5]; b.bdp = a[6]; b.bd = a[7]; b.bdd = a[8]; }
      QprDir d; d.dt = a[2]; d.dz = a[3];
      o[5] = a[9]; o[6] = a[10]; qpr_side_block(a[0], a[1], d, b, o[5], o[6]);
      o[0] = b.amax; o[1] = b.bp; o[2] = b.bdp; o[3] = b.bd; o[4] = b.bdd; put(tag, o, 7);
    } else if (!strcmp(tag, "CEN")) {
      const QprCenter c = qpr_centering(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7]); o[0] = c.mu_aff; o[1] = c.sigma; o[2] = c.smu; o[3] = c.cw; put(tag, o, 4);
    } else if (!strcmp(tag, "LEN")) {
      o[0] = qpr_step_length(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8]); put(tag, o, 1);
    } else if (!strcmp(tag, "KKT")) {
      o[0] = qpr_obj_term(a[0], a[1], a[2]); o[1] = qpr_rd_term(a[1], a[2], a[3]); put(tag, o, 2);
    } else if (!strcmp(tag, "MER")) {
      const QprMerit m = qpr_merit(a[0], a[1], a[2], a[3]); o[0] = m.gap_rel; o[1] = m.merit; put(tag, o, 2);
    } else if (!strcmp(tag, "KEEP")) {
      o[0] = qpr_keep_rule(a[0], a[1], a[2], a[3], a[4], (int)a[5]); put(tag, o, 1);
    } else if (!strcmp(tag, "REP")) {
      o[1] = a[7]; o[2] = a[8]; o[0] = qpr_repair(a[0], a[1], a[2], a[3], a[4], a[5], a[6], o[1], o[2]); put(tag, o, 3);
    } else if (!strcmp(tag, "RMER")) {
      o[0] = qpr_repaired_merit(a[0], a[1], a[2], a[3], a[4]); put(tag, o, 1);
    } else if (!strcmp(tag, "PROG")) {
      double best = a[1]; int stall = (int)a[2]; qpr_progress(a[0], best, stall); o[0] = best; o[1] = stall; put(tag, o, 2);
    } else if (!strcmp(tag, "EXIT")) {
      int flag = (int)a[7]; o[0] = qpr_exit_rule(a[0], a[1], a[2], a[3], (int)a[4], (int)a[5], (int)a[6], flag); o[1] = flag; put(tag, o, 2);
    } else if (!strcmp(tag, "SIDE")) {
      const QprSide s = qpr_working_side(a[0] != 0, a[1], a[2], a[3], a[4]); o[0] = s.lo; o[1] = s.up; o[2] = s.side();
      if (s.active() != (s.lo || s.up)) return 4;
      put(tag, o, 3);
    } else if (!strcmp(tag, "TGT")) {
      o[0] = qpr_target(a[0], a[1], a[2]); put(tag, o, 1);
    } else if (!strcmp(tag, "KVAR")) {
      o[2] = a[7]; o[3] = a[8]; o[4] = a[9];
      const QprVar s = qpr_kkt_var(a[0], a[1], a[2], a[3], a[4], a[5], a[6], o[2], o[3], o[4]); o[0] = s.r; o[1] = s.y; put(tag, o, 5);
    } else if (!strcmp(tag, "KROW")) {
      o[0] = a[6]; o[1] = a[7]; o[2] = a[8]; o[3] = a[9]; qpr_kkt_row(a[0], a[1], a[2], a[3], a[4], a[5], o[0], o[1], o[2], o[3]); put(tag, o, 4);
    } else if (!strcmp(tag, "ACC")) {
      o[0] = qpr_accept(a[0], a[1], a[2], a[3], a[4]); o[1] = qpr_correctable(a[0], a[1], a[2]); o[2] = qpr_correct_by_add(a[1]);
      o[3] = qpr_one_more_step(a[0]); o[4] = qpr_refined_merit(a[0], a[1], a[3], a[4]); put(tag, o, 5);
    } else if (!strcmp(tag, "ADD")) {
      const QprAdd s = qpr_add_score(a[0], a[1], a[2], a[3] != 0); o[0] = s.score; o[1] = s.lower; o[2] = s.side(); put(tag, o, 3);
    } else if (!strcmp(tag, "DROP")) {
      o[0] = qpr_drop_score(a[0], a[1], a[2] != 0); put(tag, o, 1);
    } else if (!strcmp(tag, "CLAMP")) {
      o[0] = qpr_clamp_multiplier(a[0], a[1]); put(tag, o, 1);
    } else return 5;
    free(a);
  }
  fclose(f);
  return 0;
}
"""


def _bits(v):
    v = float(v)
    return "nan" if v != v else struct.pack("<d", v)


def test_host_build_of_the_rules_matches_numpy_under_sanitizers(tmp_path):
    """csrc/qp_rules.h on the host (g++ -O1 -ffp-contract=off -fsanitize=address,undefined) against tests/qp_rules_numpy.py: every output
    of every case bit for bit (a NaN equals a NaN); the sanitizers report nothing; every tag and every exit / acceptance code occurs."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed for the host build"
    (tmp_path / "rules_main.cpp").write_text(HOST_MAIN)
    (tmp_path / "cases.txt").write_text("".join("%s %s\n" % (c[0], " ".join(repr(float(v)) for v in c[1:])) for c in CASES))
    exe = tmp_path / "rules_main"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",   # (the runtimes inside the program: nothing to preload)
                           "-I", os.path.join(ROOT, "fsae-mpc_amd", "csrc"), str(tmp_path / "rules_main.cpp"), "-o", str(exe)])
    run = subprocess.run(["timeout", "-k", "2", "20", str(exe), str(tmp_path / "cases.txt")], capture_output=True, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    lines = [l.split() for l in run.stdout.strip().split("\n")]
    const = [float.fromhex(v) for v in lines[0][1:]]
    assert lines[0][0] == "CONST" and const == [qr.GAMMA_F, qr.STEP_BACKOFF, qr.AMAX_UNSET, qr.AMAX_SET, qr.CORRECTOR_MIN_STEP, qr.MU_FLOOR, qr.PROGRESS,
                                                qr.STALL_SAVED, qr.STALL_UNSAVED, qr.DIVERGED_X, qr.DIVERGED_Z, qr.INFEASIBLE_RP, qr.RHO, qr.PIN,
                                                qr.ACCEPT_RD, qr.RESTEP_RD]
    assert len(lines) == len(CASES) + 1
    seen = {}
    with np.errstate(all="ignore"):
        for case, got in zip(CASES, lines[1:]):
            ref = qr.RULES[case[0]](*case[1:])
            out = [float.fromhex(v) for v in got[1:]]
            assert got[0] == case[0] and len(out) == len(ref), (case, got)
            assert [_bits(v) for v in out] == [_bits(v) for v in ref], (case, out, [float(v) for v in ref])
            seen.setdefault(case[0], []).append(out)
    assert set(seen) == set(qr.RULES)
    # the cases reach what they were chosen for
    assert {o[0] for o in seen["ACC"]} == {0.0, -1.0, -2.0, -3.0, -4.0, -5.0}
    assert {(o[0], o[1]) for o in seen["EXIT"]} == {(0.0, 1.0), (1.0, -1.0), (1.0, -2.0), (1.0, -3.0), (1.0, 1.0), (1.0, 2.0), (1.0, 5.0)}
    assert {o[0] for o in seen["KEEP"]} == {0.0, 1.0, 2.0, 3.0}
    assert {o[2] for o in seen["SIDE"]} == {0.0, 1.0, -1.0} and {o[1] for o in seen["ADD"]} == {0.0, 1.0}
    assert any(o[1] == inf for o in seen["MER"]) and all(o[1] != 0.0 for o in seen["MER"])
    assert {o[3] for o in seen["CEN"]} == {0.0, 1.0} and any(o[1] == 1.0 for o in seen["CEN"]) and any(o[1] == 0.0 for o in seen["CEN"])
    assert any(o[0] == 1e300 for o in seen["BLK"]) and any(o[0] == 0.5 and o[1] == 9.0 for o in seen["BLK"])   # unset; a tie keeps the first pair
