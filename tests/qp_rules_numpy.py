"""numpy restatement of csrc/qp_rules.h, the scalar rules of the batched QP solve: every function here repeats its C++ twin operation
for operation on IEEE doubles (np.float64 scalars; fmax / fmin drop NaN operands like the C functions), so that a host build of the
header with FMA contraction off returns the same bits (tests/test_qp_rules_cpu.py)."""
import numpy as np

F = np.float64
INF = F(np.inf)
fmax, fmin, fabs = np.fmax, np.fmin, np.abs

GAMMA_F, STEP_BACKOFF, AMAX_UNSET, AMAX_SET = F(0.99), F(0.99999999), F(1e300), F(1e299)
CORRECTOR_MIN_STEP, MU_FLOOR, PROGRESS = F(0.05), F(1e-5), F(0.9)
STALL_SAVED, STALL_UNSAVED = 5, 25
DIVERGED_X, DIVERGED_Z, INFEASIBLE_RP = F(1e13), F(1e15), F(1e-6)
RHO, PIN = F(1e6), F(1e16)
ACCEPT_RD, ACCEPT_RP, ACCEPT_CP, ACCEPT_SG, RESTEP_RD = F(1e-8), F(1e-10), F(1e-10), F(1e-8), F(1e-4)
REFINE_ATTEMPTS = 3
KEEP_NONE, KEEP_SAVE, KEEP_REPAIR, KEEP_RETURN = 0, 1, 2, 3
ZERO, ONE, HALF = F(0.0), F(1.0), F(0.5)


def _f(*a):
    return [F(v) for v in a]


def row_weights(valid, l, u, v, tl, tu, zl, zu, s_gap, m_rp):
    l, u, v, tl, tu, zl, zu, s_gap, m_rp = _f(l, u, v, tl, tu, zl, zu, s_gap, m_rp)
    hl, hu = bool(valid) and l > -INF, bool(valid) and u < INF
    rpl = v - l - tl if hl else ZERO
    rpu = u - v - tu if hu else ZERO
    dl = zl / tl if hl else ZERO
    du = zu / tu if hu else ZERO
    ccl = dl / tl if hl else ZERO
    ccu = du / tu if hu else ZERO
    D = dl + du
    W1 = -dl * rpl + du * rpu
    W2 = (ONE / tl if hl else ZERO) - (ONE / tu if hu else ZERO)
    W3 = (zl if hl else ZERO) - (zu if hu else ZERO)
    s_gap = s_gap + ((tl * zl if hl else ZERO) + (tu * zu if hu else ZERO))
    sc = fmax(ONE, fabs(v))
    if hl:
        m_rp = fmax(m_rp, fabs(rpl) / fmax(sc, fabs(l)))
    if hu:
        m_rp = fmax(m_rp, fabs(rpu) / fmax(sc, fabs(u)))
    return [rpl, rpu, dl, du, ccl, ccu, D, W1, W2, W3, s_gap, m_rp]


def side_affine(t, z, rp, va, a_aff, s1, s2):
    t, z, rp, va, a_aff, s1, s2 = _f(t, z, rp, va, a_aff, s1, s2)
    dt = va + rp
    dz = -z - (z / t) * dt
    if dt < 0:
        a_aff = fmin(a_aff, -t / dt)
    if dz < 0:
        a_aff = fmin(a_aff, -z / dz)
    s1 = s1 + (t * dz + z * dt)
    s2 = s2 + dt * dz
    return [dt * dz / t, a_aff, s1, s2]


def side_step(t, z, rp, va, dv, smu, cw):
    t, z, rp, va, dv, smu, cw = _f(t, z, rp, va, dv, smu, cw)
    dta = va + rp
    dza = -z - (z / t) * dta
    c = smu - cw * dta * dza
    dt = dv + rp
    dz = -z + c / t - (z / t) * dt
    return [dt, dz]


def side_block(t, z, dt, dz, amax, bp, bdp, bd, bdd, q1, q2):
    t, z, dt, dz, amax, bp, bdp, bd, bdd, q1, q2 = _f(t, z, dt, dz, amax, bp, bdp, bd, bdd, q1, q2)
    if dt < 0 and -t / dt < amax:
        amax, bp, bdp, bd, bdd = -t / dt, t, dt, z, dz
    if dz < 0 and -z / dz < amax:
        amax, bp, bdp, bd, bdd = -z / dz, z, dz, t, dt
    q1 = q1 + (t * dz + z * dt)
    q2 = q2 + dt * dz
    return [amax, bp, bdp, bd, bdd, q1, q2]


def centering(gap, cnt, mu, a_aff, s1, s2, tol, fval):
    gap, cnt, mu, a_aff, s1, s2, tol, fval = _f(gap, cnt, mu, a_aff, s1, s2, tol, fval)
    mu_aff = fmax(ZERO, gap + a_aff * (s1 + a_aff * s2)) / cnt
    sigma = (mu_aff / mu) * (mu_aff / mu) * (mu_aff / mu) if mu > 0 else ZERO
    if sigma > ONE:
        sigma = ONE
    mu_floor = MU_FLOOR * tol * fmax(ONE, fabs(fval)) / cnt
    if mu > 0 and sigma < mu_floor / mu:
        sigma = fmin(ONE, mu_floor / mu)
    return [mu_aff, sigma, sigma * mu, ONE if a_aff >= CORRECTOR_MIN_STEP else ZERO]


def step_length(gap, cnt, amax, q1, q2, bp, bdp, bd, bdd):
    gap, cnt, amax, q1, q2, bp, bdp, bd, bdd = _f(gap, cnt, amax, q1, q2, bp, bdp, bd, bdd)
    gamma_a = ONE / (ONE - GAMMA_F)
    mufull = fmax(ZERO, gap + amax * (q1 + amax * q2)) / cnt / gamma_a
    a_h = (-bp + mufull / (bd + amax * bdd)) / bdp
    return [fmin(ONE, fmin(STEP_BACKOFF * amax, fmax(a_h, GAMMA_F * amax)))]


def rd_scale(hx, g, gz):
    return fmax(ONE, fmax(fabs(g), fmax(fabs(hx), fabs(gz))))


def kkt_terms(x, hx, g, gz):
    x, hx, g, gz = _f(x, hx, g, gz)
    return [HALF * x * hx + g * x, fabs(hx + g - gz) / rd_scale(hx, g, gz)]


def merit(fval, gap, rd_rel, rp_rel):
    fval, gap, rd_rel, rp_rel = _f(fval, gap, rd_rel, rp_rel)
    gap_rel = gap / fmax(ONE, fabs(fval))
    ok = fabs(fval) < INF and fabs(gap_rel) < INF
    return [gap_rel, fmax(rd_rel, fmax(rp_rel, gap_rel)) if ok else INF]


def beats_saved(m, tol_loose, saved_merit):
    return bool(F(m) <= F(tol_loose) and F(m) < F(saved_merit))


def keep_rule(m, rp_rel, gap_rel, tol_loose, saved_merit, have_saved):
    m, rp_rel, gap_rel, tol_loose, saved_merit = _f(m, rp_rel, gap_rel, tol_loose, saved_merit)
    if beats_saved(m, tol_loose, saved_merit):
        return KEEP_SAVE
    if m > tol_loose and rp_rel <= tol_loose and gap_rel <= tol_loose:
        return KEEP_REPAIR
    if have_saved and m > tol_loose:
        return KEEP_RETURN
    return KEEP_NONE


def repair(lam, p3, hx, g, l, u, v, dgap, m_rd2):
    lam, p3, hx, g, l, u, v, dgap, m_rd2 = _f(lam, p3, hx, g, l, u, v, dgap, m_rd2)
    gz = p3 + lam
    r = hx + g - gz
    lam2 = lam + r
    ok = (l > -INF) if lam2 >= 0 else (u < INF)
    if ok:
        return [lam2, dgap + fabs(r) * fmax(ZERO, v - l if lam2 >= 0 else u - v), m_rd2]
    return [lam, dgap, fmax(m_rd2, fabs(r) / rd_scale(hx, g, gz))]


def repaired_merit(rd2, rp_rel, gap, dgap, fval):
    rd2, rp_rel, gap, dgap, fval = _f(rd2, rp_rel, gap, dgap, fval)
    return [fmax(rd2, fmax(rp_rel, (gap + dgap) / fmax(ONE, fabs(fval))))]


def progress(m, best_res, stall):
    m, best_res = _f(m, best_res)
    if m < PROGRESS * best_res:
        return [m, 0]
    return [best_res, stall + 1]


def exit_rule(xn, zn, rp_prev, fval, stall, have_saved, polish, flag):
    xn, zn, rp_prev, fval = _f(xn, zn, rp_prev, fval)
    if xn > DIVERGED_X:
        return [1, -2 if rp_prev > INFEASIBLE_RP else (-3 if fval < -DIVERGED_X else -1)]
    if zn > DIVERGED_Z and rp_prev > INFEASIBLE_RP:
        return [1, -2]
    if stall > (STALL_SAVED if have_saved else STALL_UNSAVED):
        return [1, 2 if have_saved else (-2 if rp_prev > INFEASIBLE_RP else (5 if polish else 1))]
    return [0, flag]


def working_side(valid, l, u, v, lam):
    l, u, v, lam = _f(l, u, v, lam)
    lo = bool(valid) and l > -INF and lam > 0 and lam > fabs(v - l)
    up = bool(valid) and u < INF and lam < 0 and -lam > fabs(u - v)
    return [int(lo), int(up), ONE if lo else (-ONE if up else ZERO)]


def target(sd, l, u):
    sd, l, u = _f(sd, l, u)
    return [l if sd > 0 else (u if sd < 0 else ZERO)]


def kkt_var(hx, g, p1, sd, zi, l, u, m_rd, m_sg, m_rp):
    hx, g, p1, sd, zi, l, u, m_rd, m_sg, m_rp = _f(hx, g, p1, sd, zi, l, u, m_rd, m_sg, m_rp)
    r = hx + g - p1
    sc = rd_scale(hx, g, p1)
    if sd == 0.0:
        m_rd = fmax(m_rd, fabs(r) / sc)
    else:
        m_sg = fmax(m_sg, (-r if sd > 0 else r) / sc)
    viol = ZERO
    if l > -INF and zi < l:
        viol = l - zi
    if u < INF and zi > u:
        viol = fmax(viol, zi - u)
    m_rp = fmax(m_rp, viol / fmax(ONE, fabs(zi)))
    return [r, r if sd != 0.0 else ZERO, m_rd, m_sg, m_rp]


def kkt_row(l, u, v, y, sd, tgt, m_rp, m_sg, m_cp, fl2):
    l, u, v, y, sd, tgt, m_rp, m_sg, m_cp, fl2 = _f(l, u, v, y, sd, tgt, m_rp, m_sg, m_cp, fl2)
    sc = fmax(ONE, fabs(v))
    if l > -INF:
        sc = fmax(sc, fabs(l))
    if u < INF:
        sc = fmax(sc, fabs(u))
    viol = ZERO
    if sd != 0.0:
        viol = fabs(v - tgt)
        m_cp = fmax(m_cp, fabs(y) * viol)
    if l > -INF and v < l:
        viol = fmax(viol, l - v)
    if u < INF and v > u:
        viol = fmax(viol, v - u)
    m_rp = fmax(m_rp, viol / sc)
    m_sg = fmax(m_sg, (-y if sd > 0 else (y if sd < 0 else ZERO)) / fmax(ONE, fabs(y)))
    fl2 = fl2 + ZERO * (v + y)
    return [m_rp, m_sg, m_cp, fl2]


def accept(m_rd, m_rp, m_sg, m_cp, f2):
    """[code, correctable, correct by add, one more step, merit of the accepted point]"""
    m_rd, m_rp, m_sg, m_cp, f2 = _f(m_rd, m_rp, m_sg, m_cp, f2)
    finite = bool(fabs(f2) < INF)
    pok = m_rd <= ACCEPT_RD and m_rp <= ACCEPT_RP and m_cp <= ACCEPT_CP * fmax(ONE, fabs(f2)) and m_sg <= ACCEPT_SG and finite
    if pok:
        code = 0
    else:
        code = -5 if not finite else (-1 if not m_rd <= ACCEPT_RD else (-2 if not m_rp <= ACCEPT_RP else (-4 if not m_sg <= ACCEPT_SG else -3)))
    correctable = bool(m_rd <= ACCEPT_RD and (m_rp > ACCEPT_RP or m_sg > ACCEPT_SG))
    one_more = bool((not m_rd <= ACCEPT_RD) and m_rd <= RESTEP_RD)
    return [code, int(correctable), int(m_rp > ACCEPT_RP), int(one_more), fmax(m_rd, fmax(m_rp, m_cp / fmax(ONE, fabs(f2))))]


def add_score(l, u, v, a_row):
    l, u, v = _f(l, u, v)
    sc = fmax(ONE, fabs(v))
    if a_row:
        if l > -INF:
            sc = fmax(sc, fabs(l))
        if u < INF:
            sc = fmax(sc, fabs(u))
    vl = (l - v) / sc if l > -INF else -ONE
    vu = (v - u) / sc if u < INF else -ONE
    return [fmax(vl, vu), int(vl >= vu), ONE if vl >= vu else -ONE]


def drop_score(sd, y, a_row):
    sd, y = _f(sd, y)
    sc = fmax(ONE, fabs(y)) if a_row else ONE
    return [(-y if sd > 0 else y) / sc]


def clamp_multiplier(sd, y):
    sd, y = _f(sd, y)
    return [fmax(y, ZERO) if sd > 0 else (fmin(y, ZERO) if sd < 0 else ZERO)]


RULES = dict(ROW=row_weights, AFF=side_affine, STEP=side_step, BLK=side_block, CEN=centering, LEN=step_length, KKT=kkt_terms, MER=merit,
             KEEP=lambda *a: [keep_rule(*a[:5], int(a[5]))], REP=repair, RMER=repaired_merit,
             PROG=lambda m, b, s: progress(m, b, int(s)), EXIT=lambda xn, zn, rp, fv, st, hs, po, fl: exit_rule(xn, zn, rp, fv, int(st), int(hs), int(po), int(fl)),
             SIDE=lambda valid, *a: working_side(int(valid), *a), TGT=target, KVAR=kkt_var, KROW=kkt_row, ACC=accept,
             ADD=lambda l, u, v, a: add_score(l, u, v, int(a)), DROP=lambda sd, y, a: drop_score(sd, y, int(a)), CLAMP=clamp_multiplier)
RULES["ROW"] = lambda valid, *a: row_weights(int(valid), *a)
