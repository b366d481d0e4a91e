"""GPU tests of the QP VJP kernel (csrc/qp_sens.hip, fsae_mpc_amd.qp_vjp / QpFunction) off the three LTV-MPC shapes: the generic QP
families of tests/qp_families.py on both sides of the switch of the factor M from LDS to the workspace slot (np = 128), with nF or
nW a multiple of 16, no working row at all, nC = 0 and nC around the 64-row trips of the compaction and the 256-row stride of the
row loops, a free variable without curvature, equality rows and a fixed variable, row scales over eight decades, an all-zero
cotangent column, shared_HA, the -1 paths (nW > nF, dependent working rows, a singular M) and what they leave in a slot for the next
instance, the autograd wrapper, and the step VJP off N = 40.

References: closed forms (families F and E) and the dense numpy adjoint (tests/sens_numpy.py), compared through sens_numpy.compare
and sens_numpy.residual -- the tolerance rule and the 1e-9 residual bound of tests/test_sens_gpu.py, nothing new.
tests/test_sens_shapes_cpu.py shows on the CPU that the references agree with each other and with differences, and that the
conditions under which a derivative is demanded here hold.  Each case prints a line starting SENSSHAPES before it asserts;
profiles/sens_shapes/README.md records them."""
import json

import numpy as np
import pytest

import qp_families as qf
import sens_numpy as sn
from test_ltv_sens_gpu import check_feedback_gain, check_step_vjp
from test_sens_shapes_cpu import B, OUT_KEYS, ROW_EDGE_NC, ROW_EDGE_NV, R_DEPENDENT_52_70, closed_form, cotangents, vjp_conditions

pytestmark = pytest.mark.gpu

RESID_TOL = 1e-9
WANT_A_MAX = 20000          # Abar is asked for where nV nC <= 20 000


@pytest.fixture(scope="module")
def fm():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import fsae_mpc_amd
    return fsae_mpc_amd


@pytest.fixture(scope="module")
def torch_():
    import torch
    return torch


@pytest.fixture(scope="module")
def track(fm):
    return fm.Track.load("fsg2019")


def _dev(torch, a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _qdev(torch, q):
    return {k: _dev(torch, q[k]) for k in qf.KEYS}


def _forward_gpu(fm, torch, q, **kw):
    d = _qdev(torch, q)
    r = fm.qp_solve_batch_device(d["H"], d["g"], d["A"], d["lb"], d["ub"], d["lbA"], d["ubA"], want_lambda=True, want_aux=True, **kw)
    torch.cuda.synchronize()
    return {k: r[k].cpu().numpy() for k in ("x", "lam", "exitflag", "polished")}


def _forward_oracle(orc, q):
    r = orc.qp_solve_batch_aux(*[q[k] for k in qf.KEYS])
    return {k: r[k] for k in ("x", "lam", "exitflag", "polished")}


def _vjp(fm, torch, q, r, xbar, fbar, sel=None, **kw):
    """qp_vjp on numpy inputs (q: stacked batch, r: x, lam, exitflag, polished; sel: a slice of instances), numpy outputs."""
    s = slice(None) if sel is None else sel
    d = {k: _dev(torch, q[k] if kw.get("shared_HA") and k in ("H", "A") else q[k][s]) for k in qf.KEYS}
    out = fm.qp_vjp(d["H"], d["g"], d["A"], d["lb"], d["ub"], d["lbA"], d["ubA"], _dev(torch, r["x"][s]), _dev(torch, r["lam"][s]),
                    _dev(torch, r["exitflag"][s], np.int32), _dev(torch, r["polished"][s], np.int32), _dev(torch, xbar[s]),
                    None if fbar is None else _dev(torch, fbar[s]), **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _exact(n, flag=0, pol=1):
    return dict(exitflag=np.full(n, flag, dtype=np.int32), polished=np.full(n, pol, dtype=np.int32))


class Figures:
    """What one case prints: status histogram, worst error over tolerance, worst residual, nF and nW ranges, compared and left-out
    instances by reason."""

    def __init__(self, group, case):
        self.fig = dict(group=group, case=case, status={}, worst=0.0, resid=0.0, nF=[10 ** 9, -1], nW=[10 ** 9, -1], compared=0, left_out={})
        self.failures = []

    def status(self, st):
        self.fig["status"] = {str(int(s)): int(c) for s, c in zip(*np.unique(st, return_counts=True))}

    def sizes(self, c):
        for key in ("nF", "nW"):
            self.fig[key] = [min(self.fig[key][0], c[key]), max(self.fig[key][1], c[key])]

    def left(self, reason):
        self.fig["left_out"][reason] = self.fig["left_out"].get(reason, 0) + 1

    def fail(self, *what):
        self.failures.append(what)

    def done(self, **extra):
        self.fig.update(extra)
        if self.fig["nF"][1] < 0:          # no instance went through _judge
            self.fig["nF"] = self.fig["nW"] = None
        print("SENSSHAPES " + json.dumps(self.fig))
        assert not self.failures, self.failures[:6]
        return self.fig


def _slice(got, b, c, keys):
    return {key: got[key][b, c] for key in keys if key in got}


def _all_zero(got, b):
    return not any(np.any(got[key][b]) for key in got if key != "status")


def _judge(F, q, r, got, xbar, fbar, conds, dup=(3, 4), refs=None, only=None):
    """The rules of group C on every instance (or on those of `only`); groups A, B and E are special cases of them.

    Status: -2 exactly where the forward's flag != 0 (zeros); a computed status is 2 exactly where polished <= 0, and 1 only where
    a working-set multiplier is <= tol (1 + |lambda|_inf).  With the working set of the rule recomputed in numpy from the same x and
    lambda (conds): independent working rows on the free columns and nW <= nF -- status >= 0, every output compared with the
    reference (sens_numpy.adjoint, or refs[b][c]) through sens_numpy.compare and the residual of the returned (w, mu) <= 1e-9;
    nW > nF -- status -1, every output exactly zero; dependent rows with nW <= nF -- either status -1 with zeros, or a computed
    status with the residual <= 1e-9 and gbar equal to the least-squares gbar (w is unique; the split of mu over duplicate rows is
    not: where the dependency is exactly the duplicate pair `dup`, the sum of their mu is compared)."""
    st = got["status"]
    keys = [key for key in OUT_KEYS if key in got]
    k = xbar.shape[1]
    F.status(st)
    for b in (range(len(st)) if only is None else only):
        c_, s = conds[b], int(st[b])
        qb = (q["H"][b].T, q["g"][b], q["A"][b].T)
        x, lam = r["x"][b], r["lam"][b]
        if r["exitflag"][b] != 0:
            F.left("forward flag != 0")
            if s != -2 or not _all_zero(got, b):
                F.fail(b, "flag != 0 needs -2 and zeros", s)
            continue
        F.sizes(c_)
        if s == -2 or s not in (-1, 0, 1, 2):
            F.fail(b, "status", s)
            continue
        if s >= 0 and ((s == 2) != (r["polished"][b] <= 0) or (s == 1 and not c_["weak"])):
            F.fail(b, "status against polished / weak", s, int(r["polished"][b]), c_["weak"])
        if s == -1 and not _all_zero(got, b):
            F.fail(b, "-1 without zeros")
        over, dep = c_["nW"] > c_["nF"], not c_["independent"]
        if over:
            F.left("nW > nF (-1)")
            if s != -1:
                F.fail(b, "nW > nF needs -1", s, c_["nW"], c_["nF"])
            continue
        if dep and s == -1:
            F.left("dependent (-1)")
            continue
        if s == -1:
            F.fail(b, "independent working rows, nW <= nF, but -1", c_["nW"], c_["nF"], c_["rank"], c_["cond"])
            continue
        F.fig["compared"] += 1
        if dep:
            F.fig["dependent_computed"] = F.fig.get("dependent_computed", 0) + 1
        n = len(x)
        for c in range(k):
            g_ = _slice(got, b, c, keys)
            e, parts = sn.residual(g_, *qb, x, xbar[b, c], fbar[b, c])
            F.fig["resid"] = max(F.fig["resid"], e)
            if not e <= RESID_TOL:
                F.fail(b, c, "residual", e, parts)
            if refs is not None:
                ref = refs[b][c]
            else:
                ref = sn.adjoint(*qb, x, lam, c_["ws"], xbar[b, c], fbar[b, c], lstsq=dep)
            if dep:
                cmp_got, cmp_ref = dict(g=g_["g"]), ref
                wr = c_["ws"][n:]
                if c_["rank"] == c_["nW"] - 1 and len(wr) > max(dup) and wr[dup[0]] != 0 and wr[dup[0]] == wr[dup[1]] \
                        and np.array_equal(qb[2][dup[0]], qb[2][dup[1]]):
                    side = "lbA" if wr[dup[0]] < 0 else "ubA"
                    cmp_got[side] = np.array([g_[side][dup[0]] + g_[side][dup[1]]])
                    cmp_ref = dict(ref)
                    cmp_ref[side] = np.array([ref[side][dup[0]] + ref[side][dup[1]]])
            else:
                cmp_got, cmp_ref = g_, ref
            e, where = sn.compare(cmp_got, cmp_ref, *qb, x, lam, xbar[b, c], fbar[b, c])
            F.fig["worst"] = max(F.fig["worst"], e)
            if not e <= 1.0:
                F.fail(b, c, "error over tolerance", e, where)


def _cot(nV, nC, n, k=2):
    """k cotangent columns with fbar for n instances."""
    rng = np.random.default_rng([5, nV, nC])
    return rng.standard_normal((n, k, nV)), rng.standard_normal((n, k))


# ---- A. independent of the forward solver: closed forms ---------------------------------------------------------------------------

@pytest.mark.parametrize("family,nV,nC", [(f, n, m) for f in ("F", "E") for n, m in qf.VJP_SHAPES + (qf.SHAPES_F_ONLY if f == "F" else [])])
def test_A_closed_forms(fm, torch_, family, nV, nC):
    """qp_vjp takes x, lambda, exitflag and polished as inputs: x_star, lam_star, flag 0 and polished 1 from numpy.  F: no working
    row (the SYRK has no k-loop; nF = nV, at (16, 16) and (96, 130) without identity padding; nC = 0 at (20, 0)); E: equality rows,
    the side chosen by the sign of lambda alone.  k = 3: random xbar and fbar | random xbar, fbar = 0 | all zero."""
    q = qf.batch(family, nV, nC, B)
    r = dict(x=q["x_star"], lam=q["lam_star"], **_exact(B))
    xbar, fbar = cotangents(B, 3, nV, 1)
    got = _vjp(fm, torch_, q, r, xbar, fbar, want_H=True, want_A=True)
    conds = vjp_conditions(q, r["x"], r["lam"], r["exitflag"], r["polished"])
    refs = []
    for b in range(B):
        qb = {key: (q[key][b].T if key in ("H", "A") else q[key][b]) for key in qf.KEYS}
        qb.update(x_star=q["x_star"][b], lam_star=q["lam_star"][b])
        refs.append([dict(closed_form(qb, xbar[b, c], fbar[b, c]), cond=conds[b]["cond"]) for c in range(3)])
    F = Figures("A closed forms", "%s (%d,%d)" % (family, nV, nC))
    _judge(F, q, r, got, xbar, fbar, conds, refs=refs)
    if not (got["status"] == 0).all():
        F.fail("status 0 on every instance", got["status"].tolist())
    lamA = q["lam_star"][:, None, nV:]
    if np.any(got["lb"]) or np.any(got["ub"]) or np.any(got["lbA"][np.broadcast_to(lamA <= 0, got["lbA"].shape)]) \
            or np.any(got["ubA"][np.broadcast_to(lamA >= 0, got["ubA"].shape)]):
        F.fail("a cotangent off the side that the sign of lambda names")
    if family == "E":
        kE = min(nC, nV // 2)
        # lbAbar + ubAbar = mu on the equality rows: one side equals mu (compared above), the other is exactly zero (above too)
        if not (np.count_nonzero(got["lbA"][:, 0] + got["ubA"][:, 0], axis=1) == kE).all():
            F.fail("every equality row has its cotangent")
    if any(np.any(got[key][:, 2]) for key in OUT_KEYS):
        F.fail("column 2 (xbar = 0, fbar = 0) is not exactly zero")
    F.done()


# ---- B. oracle forward (refined vertices) ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family,nV,nC", [(f, n, m) for f in ("S", "V") for n, m in qf.VJP_SHAPES])
def test_B_oracle_vertices(fm, torch_, orc, family, nV, nC):
    """S (a free variable without curvature) and V (staircase rows, scales over eight decades, a fixed variable) at the refined
    vertices of the CPU oracle: every instance is compared, status 0 or 1."""
    q = qf.vjp_batch(family, nV, nC, B)
    r = _forward_oracle(orc, q)
    xbar, fbar = _cot(nV, nC, B)
    got = _vjp(fm, torch_, q, r, xbar, fbar, want_H=True, want_A=nV * nC <= WANT_A_MAX)
    conds = vjp_conditions(q, r["x"], r["lam"], r["exitflag"], r["polished"])
    F = Figures("B oracle forward", "%s (%d,%d)" % (family, nV, nC))
    _judge(F, q, r, got, xbar, fbar, conds)
    if not all(c["ok"] for c in conds) or not (r["polished"] > 0).all():
        F.fail("the reference does not meet its conditions", [(c["nF"], c["nW"], c["rank"], c["cond"]) for c in conds if not c["ok"]])
    if F.fig["compared"] != B or not np.isin(got["status"], (0, 1)).all():
        F.fail("an instance was left out or has a status other than 0 / 1", got["status"].tolist())
    F.done(weak=int(sum(c["weak"] for c in conds)))


# ---- C. GPU forward, as users run it ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family,nV,nC", [(f, n, m) for f in ("F", "E", "S", "V", "R") for n, m in qf.SHAPES])
def test_C_gpu_forward(fm, torch_, family, nV, nC):
    """qp_solve_batch_device(want_lambda, want_aux) then qp_vjp, judged by the rules of _judge on every instance; R (24, 200) reaches
    nW > np on its own."""
    q = qf.batch(family, nV, nC, B)
    r = _forward_gpu(fm, torch_, q)
    xbar, fbar = _cot(nV, nC, B)
    got = _vjp(fm, torch_, q, r, xbar, fbar, want_H=True, want_A=nV * nC <= WANT_A_MAX)
    conds = vjp_conditions(q, r["x"], r["lam"], r["exitflag"], r["polished"])
    F = Figures("C GPU forward", "%s (%d,%d)" % (family, nV, nC))
    _judge(F, q, r, got, xbar, fbar, conds)
    F.done(dependent=int(sum(not c["independent"] and c["nW"] <= c["nF"] for c in conds)), refined=int((r["polished"] > 0).sum()))


# ---- D. constructed degenerate vertices ------------------------------------------------------------------------------------------

def _one(H, g, A, lb, ub, lbA, ubA, x, lam):
    n = len(g)
    A = np.asarray(A, dtype=np.float64).reshape(-1, n)
    q = dict(H=np.asarray(H, dtype=np.float64).T[None], g=np.asarray(g, dtype=np.float64)[None], A=np.ascontiguousarray(A.T)[None],
             lb=np.asarray(lb, dtype=np.float64)[None], ub=np.asarray(ub, dtype=np.float64)[None],
             lbA=np.asarray(lbA, dtype=np.float64).reshape(1, -1), ubA=np.asarray(ubA, dtype=np.float64).reshape(1, -1))
    r = dict(x=np.asarray(x, dtype=np.float64)[None], lam=np.asarray(lam, dtype=np.float64)[None], **_exact(1))
    return q, r


def test_D_constructed_degenerate_vertices(fm, torch_):
    """x and lambda made by hand (all valid calls): three active rows on two variables (nW > nF); two identical active rows; a free
    variable without curvature that no working row touches (M singular) and the same variable touched by one working row (the
    known answer of its 2 x 2 system); a fixed variable with lambda > 0, then < 0."""
    torch = torch_
    F = Figures("D constructed", "n <= 3")
    inf = np.inf
    # n = 2, three active upper sides: status -1, zeros
    A = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    x, lamA = np.array([1.0, 1.0]), np.array([-1.0, -1.0, -1.0])
    q, r = _one(np.eye(2), A.T @ lamA - x, A, [-10, -10], [10, 10], [-inf] * 3, A @ x, x, np.concatenate([np.zeros(2), lamA]))
    xbar, fbar = _cot(2, 3, 1)
    got = _vjp(fm, torch, q, r, xbar, fbar, want_H=True, want_A=True)
    conds = vjp_conditions(q, r["x"], r["lam"], r["exitflag"], r["polished"])
    assert conds[0]["nW"] == 3 and conds[0]["nF"] == 2
    _judge(F, q, r, got, xbar, fbar, conds)
    if got["status"][0] != -1:
        F.fail("three rows on two variables", int(got["status"][0]))
    # n = 3, two identical active rows: the either / or of dependent rows
    A = np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 0.0]])
    H = np.diag([1.0, 2.0, 3.0])
    x, lamA = np.array([0.5, 0.5, 0.0]), np.array([-1.0, -1.0])
    q, r = _one(H, A.T @ lamA - H @ x, A, [-10] * 3, [10] * 3, [-inf] * 2, A @ x, x, np.concatenate([np.zeros(3), lamA]))
    xbar, fbar = _cot(3, 2, 1)
    got = _vjp(fm, torch, q, r, xbar, fbar, want_H=True, want_A=True)
    conds = vjp_conditions(q, r["x"], r["lam"], r["exitflag"], r["polished"])
    assert conds[0]["nW"] == 2 and conds[0]["rank"] == 1
    _judge(F, q, r, got, xbar, fbar, conds, dup=(0, 1))
    st_dup = int(got["status"][0])
    # a free variable with H_ii = 0: untouched by the working row -> M is singular, -1 and zeros; touched -> status 0
    H = np.diag([1.0, 0.0])
    for A, x in (([[1.0, 0.0]], [1.0, 0.3]), ([[1.0, 1.0]], [0.4, 0.6])):
        A, x = np.array(A), np.array(x)
        lamA = np.array([-2.0])
        q, r = _one(H, A.T @ lamA - H @ x, A, [-10] * 2, [10] * 2, [-inf], A @ x, x, np.concatenate([np.zeros(2), lamA]))
        xbar, fbar = _cot(2, 1, 1)
        fbar[:] = 0.0
        got = _vjp(fm, torch, q, r, xbar, fbar, want_H=True, want_A=True)
        conds = vjp_conditions(q, r["x"], r["lam"], r["exitflag"], r["polished"])
        if A[0, 1] == 0.0:
            if got["status"][0] != -1 or not _all_zero(got, 0):
                F.fail("zero curvature, untouched: -1 and zeros", int(got["status"][0]))
            F.left("singular M (-1)")
        else:
            _judge(F, q, r, got, xbar, fbar, conds)
            for c in range(2):
                # w = (w0, -w0) with w0 + mu = xbar0, mu = xbar1
                x0b, x1b = xbar[0, c]
                want_g, want_mu = np.array([x1b - x0b, x0b - x1b]), x1b
                e = max(np.abs(got["g"][0, c] - want_g).max(), abs(got["ubA"][0, c, 0] - want_mu)) / max(1.0, np.abs(xbar[0, c]).max())
                if got["status"][0] != 0 or not e <= 1e-12 or got["lbA"][0, c, 0] != 0.0:
                    F.fail("zero curvature, touched: known answer", int(got["status"][0]), e)
    # a fixed variable (lb = ub): the side is the sign of lambda alone
    H = np.array([[2.0, 0.5], [0.5, 1.0]])
    x = np.array([0.7, -0.2])
    xbar, fbar = _cot(2, 0, 1)
    fbar[:] = 0.0
    sides = {}
    for sgn in (1.0, -1.0):
        lam = np.array([3.0 * sgn, 0.0])
        q, r = _one(H, lam - H @ x, np.zeros((0, 2)), [0.7, -10], [0.7, 10], [], [], x, lam)
        got = _vjp(fm, torch, q, r, xbar, fbar, want_H=True)
        conds = vjp_conditions(q, r["x"], r["lam"], r["exitflag"], r["polished"])
        _judge(F, q, r, got, xbar, fbar, conds)
        sides[sgn] = got
        for c in range(2):
            w1 = xbar[0, c, 1] / H[1, 1]
            mu0 = xbar[0, c, 0] - H[0, 1] * w1
            on, off = ("lb", "ub") if sgn > 0 else ("ub", "lb")
            if got["status"][0] != 0 or abs(got[on][0, c, 0] - mu0) > 1e-12 * max(1.0, abs(mu0)) or np.any(got[off]) or got[on][0, c, 1] != 0.0:
                F.fail("fixed variable", sgn, c, int(got["status"][0]), got[on][0, c].tolist(), got[off][0, c].tolist(), mu0)
    if not np.array_equal(sides[1.0]["lb"], sides[-1.0]["ub"]) or not np.array_equal(sides[1.0]["g"], sides[-1.0]["g"]):
        F.fail("the two sides of the fixed variable carry different values")
    F.done(duplicate_rows_status=st_dup)


# ---- E. row-count edges ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nC", ROW_EDGE_NC)
def test_E_row_count_edges(fm, torch_, orc, nC):
    """V at nV = 35 with nC = 0 (A == nullptr), 1, and around 64 and 256; oracle forward.  With more rows than variables many
    vertices are degenerate: every instance goes through the rules of _judge (tests/test_sens_shapes_cpu.py has the counts)."""
    nV = ROW_EDGE_NV
    q = qf.vjp_batch("V", nV, nC, B)
    r = _forward_oracle(orc, q)
    xbar, fbar = _cot(nV, nC, B)
    got = _vjp(fm, torch_, q, r, xbar, fbar, want_H=True, want_A=True)
    conds = vjp_conditions(q, r["x"], r["lam"], r["exitflag"], r["polished"])
    F = Figures("E row-count edges", "V (%d,%d)" % (nV, nC))
    _judge(F, q, r, got, xbar, fbar, conds)
    if nC <= 1 and F.fig["compared"] != B:
        F.fail("nC <= 1: every instance compared")
    F.done(conditions_hold=int(sum(c["ok"] for c in conds)))


# ---- F. shared_HA -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nV,nC", [(52, 70), (130, 65)])
def test_F_shared_HA_is_bit_identical_to_stacked(fm, torch_, orc, nV, nC):
    qps = [qf.make("V", nV, nC, i, ha_inst=0) for i in range(6)]
    q, qs = qf.stack(qps), qf.stack(qps, shared_HA=True)
    assert qs["H"].shape == (nV, nV) and qs["A"].shape == (nV, nC)
    r = _forward_oracle(orc, q)
    xbar, fbar = _cot(nV, nC, 6)
    a = _vjp(fm, torch_, q, r, xbar, fbar)
    b = _vjp(fm, torch_, qs, r, xbar, fbar, shared_HA=True)
    F = Figures("F shared_HA", "V (%d,%d) x 6" % (nV, nC))
    F.status(b["status"])
    _judge(F, q, r, b, xbar, fbar, vjp_conditions(q, r["x"], r["lam"], r["exitflag"], r["polished"]))
    for key in ("g", "lb", "ub", "lbA", "ubA", "status"):
        if not np.array_equal(a[key], b[key]):
            F.fail("shared_HA differs from stacked", key)
    F.done()
    with pytest.raises(fm._lib.FsaempcError):
        _vjp(fm, torch_, qs, r, xbar, fbar, shared_HA=True, want_H=True)


# ---- G. slot reuse and isolation ----------------------------------------------------------------------------------------------------

def test_G_slot_reuse_and_isolation(fm, torch_):
    """B = 600 at (52, 70): 512 slots, so 88 of them serve two instances.  Instance 50 is infeasible, 60 has a NaN in g, 70 is an R
    instance with dependent working rows; 562, 572 and 582 reuse their slots.  Solo calls (B = 1) are bit-identical in every
    output, and so are two runs of the batch."""
    nV, nC, Bg = 52, 70, 600
    qps = [qf.make("VSE"[i % 3], nV, nC, i) for i in range(Bg)]
    qps[50] = qf.make_infeasible(nV, nC, 50)
    qps[60]["g"][5] = np.nan
    qps[70] = qf.make("R", nV, nC, R_DEPENDENT_52_70)
    q = qf.stack(qps)
    r = _forward_gpu(fm, torch_, q)
    xbar, fbar = _cot(nV, nC, Bg)
    got = _vjp(fm, torch_, q, r, xbar, fbar, want_H=True, want_A=True)
    again = _vjp(fm, torch_, q, r, xbar, fbar, want_H=True, want_A=True)
    F = Figures("G slot reuse", "VSE (52,70) x 600")
    sel = [0, 1, 49, 50, 51, 60, 70, 562, 572, 582, 599]
    qs = {k: q[k][sel] for k in qf.KEYS}
    conds = dict(zip(sel, vjp_conditions(qs, r["x"][sel], r["lam"][sel], r["exitflag"][sel], r["polished"][sel])))
    _judge(F, q, r, got, xbar, fbar, conds, only=sel)
    for b in (50, 60):
        if got["status"][b] != -2 or not _all_zero(got, b):
            F.fail("bad instance", b, int(got["status"][b]), int(r["exitflag"][b]))
    for key in got:
        if not np.array_equal(got[key], again[key], equal_nan=True):
            F.fail("two runs differ", key)
    for b in (0, 1, 49, 51, 562, 572, 582, 599):
        solo = _vjp(fm, torch_, q, r, xbar, fbar, sel=slice(b, b + 1), want_H=True, want_A=True)
        for key in got:
            if not np.array_equal(solo[key][0], got[key][b], equal_nan=True):
                F.fail("solo call differs", b, key)
    F.done(status_70=int(got["status"][70]), dependent_70=not conds[70]["independent"])


# ---- H. autograd --------------------------------------------------------------------------------------------------------------------

def test_H_qp_function_gradients_equal_the_vjp(fm, torch_):
    torch = torch_
    nV, nC = 66, 33
    q = _qdev(torch, qf.batch("S", nV, nC, B))
    rng = np.random.default_rng(5)
    cx, cf = _dev(torch, rng.standard_normal((B, nV))), _dev(torch, rng.standard_normal(B))
    leaves = {key: q[key].clone().requires_grad_(True) for key in qf.KEYS}
    status = torch.empty(B, dtype=torch.int32, device="cuda")
    x, fval, flag, pol = fm.QpFunction.apply(*[leaves[key] for key in qf.KEYS], None, status)
    r = fm.qp_solve_batch_device(*[q[key] for key in qf.KEYS], want_lambda=True, want_aux=True)
    assert torch.equal(x, r["x"]) and torch.equal(flag, r["exitflag"])
    ((x * cx).sum() + (fval * cf).sum()).backward()
    ref = fm.qp_vjp(*[q[key] for key in qf.KEYS], r["x"], r["lam"], r["exitflag"], r["polished"], cx, cf, want_H=True, want_A=True)
    F = Figures("H autograd", "S (66,33)")
    F.status(ref["status"].cpu().numpy())
    F.done()
    assert torch.equal(status, ref["status"]) and (ref["status"] >= 0).any()
    for key in leaves:
        assert torch.equal(leaves[key].grad, ref[key]), key


# ---- I. the step VJP off N = 40 ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model,N,nV", [(1, 63, 130), (1, 62, 128), (0, 9, 19)])
def test_I_step_vjp_off_N40(fm, torch_, track, model, N, nV):
    """tests/test_ltv_sens_gpu.py's comparisons of feedback_gain and ltv_step_vjp with central differences (1e-6 on every instance
    whose working set holds at +-h, a quarter of the comparisons at least) at dynamic N = 63 (nV = 130: workgroup forward, M in the
    slot), dynamic N = 62 (nV = 128: the last LDS size) and kinematic N = 9 (nV = 19)."""
    a = check_feedback_gain(fm, torch_, track, model, N, 16)
    b = check_step_vjp(fm, torch_, track, model, N, 16)
    assert a["nV"] == nV
    print("SENSSHAPES " + json.dumps(dict(group="I step VJP", case="%s N=%d nV=%d" % ("dyn" if model else "kin", N, nV), feedback_gain=a, step_vjp=b)))
