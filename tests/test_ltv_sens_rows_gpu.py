"""GPU tests of the step VJP (fsaempc_ltv_step_vjp_batch_device: ltv_vjp_pre_kernel, the QP VJP kernel, ltv_vjp_chain_kernel of
csrc/ltv_build.hip; Python ltv_step_vjp / ltv_step_diff) against a dense reference of its own, tests/ltv_sens_numpy.py, entry by
entry on every instance with a computed status (0, 1 or 2) whose working set determines its multipliers (independent rows on the
free columns, nW <= nF: where test_sens_shapes_gpu._judge demands every output) -- not only where a working set survives +-h, which
is all that the comparisons with differences of tests/test_ltv_sens_gpu.py can use.  The inputs (tests/ltv_sens_cases.py) put a multiplier on every row family of
the constraint block, so the unit coefficients of the v and delta rows and the -Crow'(lbAbar + ubAbar) term of every family
reach the chain with a non-zero cotangent; the cotangent sets pass sbar, each cotangent alone (the null-pointer branches of both
kernels) and k = 3 columns; an infeasible batch pins the zeros of status -2.

The reference differentiates LtvBatch.build_qp -- the QP that the VJP entry rebuilds -- by differencing it, and takes z and lambda
from ltv_step_lambda.  The tolerance of an output entry is ltv_sens_numpy.step_vjp's: sens_numpy.compare's tolerances of gbar,
lbAbar and ubAbar (which the QP stage has to meet in tests/test_sens_gpu.py) weighted by the absolute Jacobian entries that
multiply them, plus 100 eps of the entry's absolute terms.  tests/test_ltv_sens_cpu.py checks the reference against differences of
the CPU oracle's step and the conditions on the inputs.  Each comparison prints a line starting LTVSENS before it asserts;
profiles/sens_shapes/README.md records them."""
import json

import numpy as np
import pytest

import ltv_sens_cases as lc
import ltv_sens_numpy as ln
import sens_numpy as sn
from test_ltv_sens_gpu import _dev, _np
from test_sens_shapes_cpu import WEAK_TOL

pytestmark = pytest.mark.gpu

_CACHE = {}


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
    return fm.Track.load(lc.TRACK)


class GpuCase:
    """One batch on the device: the LtvBatch, its inputs, the forward with multipliers, the QP of LtvBatch.build_qp and its
    Jacobians in x0 and x_ref (differences of build_qp), all computed once; vjp() calls ltv_step_vjp on numpy cotangents and
    reference() the numpy restatement on the instances of comparable(), cached per cotangent set."""

    def __init__(self, fm, torch, track, model, N, d):
        self.fm, self.torch, self.model, self.N = fm, torch, model, N
        self.nx, self.ns, self.nV, self.nC = lc.dims(model, N)
        B = self.B = len(d["x0"])
        self.mpc = fm.LtvBatch(model, N, lc.DT, track, B)
        assert (self.mpc.nx, self.mpc.ns, self.mpc.nV, self.mpc.nC) == lc.dims(model, N)
        self.x0n, self.xrn = d["x0"], d["x_ref"].reshape(B, -1)
        self.x0, self.xr, self.xl, self.ul = (_dev(torch, np.asarray(a).reshape(B, -1)) for a in (d["x0"], d["x_ref"], d["x_lin"], d["u_lin"]))
        self.fwd = fm.ltv_step_lambda(self.mpc, self.x0, self.xr, self.xl, self.ul)
        self.f = {k: _np(v) for k, v in self.fwd.items()}
        self.z = np.concatenate([self.f["u_opt"], self.f["slack"]], axis=1)
        self.q = {k: _np(v) for k, v in self.mpc.build_qp(self.x0, self.xr, self.xl, self.ul).items()}
        self.jac = ln.build_jacobians(self._build, self.x0n, self.xrn)
        self._ref, self._comparable = {}, None

    def _build(self, x0, xr):
        q = self.mpc.build_qp(_dev(self.torch, x0), _dev(self.torch, xr), self.xl, self.ul)
        return {k: _np(q[k]) for k in ln.MOVING}

    def vjp(self, cot, squeeze=False, **kw):
        """ltv_step_vjp on the cotangents of `cot` ((B, k, *); squeeze: k = 1 passed without the column axis).  numpy outputs."""
        up = lambda v: None if v is None else _dev(self.torch, v[:, 0] if squeeze else v)
        r = self.fm.ltv_step_vjp(self.mpc, self.fwd, self.x0, self.xr, self.xl, self.ul, **{k: up(v) for k, v in cot.items()}, **kw)
        self.torch.cuda.synchronize()
        return {k: (None if v is None else _np(v)) for k, v in r.items()}

    def reference(self, name):
        if name not in self._ref:
            cot = lc.cotangents(self.model, self.N, self.B, name)
            self._ref[name] = ln.step_vjp(self.q, self.jac, self.z, self.f["lam"], cot, self.ns, only=np.nonzero(self.comparable())[0])
        return self._ref[name]

    def comparable(self):
        """The instances on which _judge of tests/test_sens_shapes_gpu.py demands every output of the QP VJP, whatever the status:
        forward flag 0, and the working set of the rule has independent rows on its free columns and no more rows than free
        variables.  Elsewhere the multipliers of the adjoint are not unique (or there is none), and neither is the step VJP."""
        if self._comparable is None:
            ok = self.f["exitflag"] == 0
            for b, ws in enumerate(ln.working_sets(self.q, self.z, self.f["lam"])):
                cd = sn.conditions(self.q["H"][b].T, self.q["A"][b].T, ws)
                ok[b] &= cd["rank"] == cd["nW"] and cd["nW"] <= cd["nF"]
            self._comparable = ok
        return self._comparable


def _case(fm, torch, track, model, N, infeasible=False):
    key = (model, N, infeasible)
    if key not in _CACHE:
        _CACHE[key] = GpuCase(fm, torch, track, model, N, lc.infeasible_inputs(model) if infeasible else lc.inputs(model, N))
    return _CACHE[key]


def _ratios(got, ref, sel):
    """Worst |got - ref| / tolerance over the instances of `sel`, per output; NaN counts as a miss."""
    out = {}
    for key in ("x0", "x_ref"):
        with np.errstate(invalid="ignore", divide="ignore"):
            e = np.abs(got[key][sel] - ref[key][sel]) / ref["tol_" + key][sel]
        e = np.where(np.abs(got[key][sel] - ref[key][sel]) == 0.0, 0.0, e)
        out[key] = float(np.where(np.isnan(e), np.inf, e).max()) if e.size else 0.0
    return out


def _check_statuses(c, st, got):
    """The rules of test_sens_shapes_gpu._judge that concern the step: -2 exactly where the forward failed, a computed status is
    2 exactly where polished <= 0, and a negative status gives exact zeros (status 1 only with a weakly active side: _compare)."""
    flag, pol = c.f["exitflag"], c.f["polished"]
    assert np.array_equal(st == -2, flag != 0), (st, flag)
    assert np.isin(st, (-2, -1, 0, 1, 2)).all(), st
    assert np.array_equal((st == 2), (st >= 0) & (pol <= 0)), (st, pol)
    neg = st < 0
    assert not got["x0"][neg].any() and (got["x_ref"] is None or not got["x_ref"][neg].any())


def _weak(c, ref, b):
    ws = ref["ws"][b]
    lam = c.f["lam"][b]
    return bool((np.abs(lam[ws != 0]) <= WEAK_TOL * (1.0 + np.abs(lam).max())).any())


def _family_counts(c, ref, sel):
    """Per row family: the compared instances whose lbAbar + ubAbar (column 0 of the reference's adjoint) is non-zero in it."""
    return {name: int(sum(bool(ln.row_cotangent(ref, b)[rows].any()) for b in sel)) for name, rows in lc.families(c.model, c.N).items()}


def _compare(c, name, tag="direct"):
    cot = lc.cotangents(c.model, c.N, c.B, name)
    got = c.vjp(cot)
    ref = c.reference(name)
    st = got["status"]
    _check_statuses(c, st, got)
    sel = np.nonzero((st >= 0) & c.comparable())[0]
    rat = _ratios(got, ref, sel)
    fig = dict(test=tag, case=lc.case_id((c.model, c.N)), cotangents=name, B=c.B, compared=len(sel),
               left_out={"status < 0": int((st < 0).sum()), "dependent rows or nW > nF, computed": int(((st >= 0) & ~c.comparable()).sum())},
               refused_though_comparable=int(((st == -1) & c.comparable()).sum()),
               status={str(int(s)): int(n) for s, n in zip(*np.unique(st, return_counts=True))}, worst_x0=rat["x0"], worst_x_ref=rat["x_ref"],
               families=_family_counts(c, ref, sel), cond=float(max([ref["adj"][(b, 0)]["cond"] for b in sel] or [0.0])))
    print("LTVSENS " + json.dumps(fig))
    for b in sel:
        assert st[b] != 1 or _weak(c, ref, b), (b, "status 1 without a weakly active side")
    assert fig["refused_though_comparable"] == 0, fig       # _judge: independent working rows and nW <= nF, but -1
    assert rat["x0"] <= 1.0 and rat["x_ref"] <= 1.0, fig
    return got, ref, sel, fig


# ---- direct comparison -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", lc.COTANGENT_SETS)
@pytest.mark.parametrize("case", lc.CASES, ids=lc.case_id)
def test_step_vjp_matches_the_dense_reference(fm, torch_, track, case, name):
    """x0bar and xrefbar entry by entry on every instance with status 0, 1 or 2 (_judge compares a status-2 instance with the
    adjoint on the rule's working set exactly as it does 0 and 1, so they are included), every column of the k = 3 set."""
    c = _case(fm, torch_, track, *case)
    got, ref, sel, fig = _compare(c, name)
    assert got["x0"].shape == (c.B, 3 if name == "all_k3" else 1, c.nx) and got["x_ref"].shape[2] == c.nx * c.N
    assert len(sel) >= c.B * 3 // 4, fig
    assert np.abs(ref["x0"][sel]).max() > 0 and np.abs(ref["x_ref"][sel]).max() > 0


# ---- coverage, on the GPU's own forward --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model", [0, 1])
def test_every_row_family_and_a_weakly_active_side_are_compared(fm, torch_, track, model):
    """What the N = 8 inputs are for, on the forward that the VJP is given: among the compared instances every row family has at
    least two with a non-zero lbAbar + ubAbar, three quarters of the batch are compared, a slack cotangent reaches a non-zero slack
    and at least one compared instance has status 1."""
    c = _case(fm, torch_, track, model, lc.N_ROWS)
    got, ref, sel, fig = _compare(c, "all", tag="coverage")
    assert all(n >= 2 for n in fig["families"].values()), fig
    assert len(sel) >= c.B * 3 // 4, fig
    assert (got["status"][sel] == 1).sum() >= 1, fig
    assert (np.abs(c.f["slack"][sel]) > 1e-9).any()


# ---- argument forms ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", lc.CASES, ids=lc.case_id)
def test_want_xref_false_gives_the_same_x0(fm, torch_, track, case):
    c = _case(fm, torch_, track, *case)
    for name in ("xbar", "all_k3"):
        cot = lc.cotangents(c.model, c.N, c.B, name)
        a, b = c.vjp(cot), c.vjp(cot, want_xref=False)
        assert b["x_ref"] is None and np.array_equal(a["status"], b["status"])
        assert np.array_equal(a["x0"].view(np.uint64), b["x0"].view(np.uint64))


@pytest.mark.parametrize("name", ["ubar", "xbar", "sbar", "fbar"])
@pytest.mark.parametrize("case", lc.CASES, ids=lc.case_id)
def test_a_cotangent_alone_equals_the_call_with_the_others_zero(fm, torch_, track, case, name):
    """The null-pointer branches against explicit zeros.  Both kernels and the QP VJP add the products of a zero cotangent as
    exact zeros (ltv_vjp_pre_kernel: s += Bt * 0; the QP VJP: xb + (fb != 0 ? fb * HXG : 0), -w + fb * x; the chain: p = 0, t = 2 w G
    + 2 fb w d), so the results are equal as numbers in every entry (a zero may change its sign); the call without the column
    axis ((B, n) and (B,)) returns the same numbers as the one with it."""
    c = _case(fm, torch_, track, *case)
    cot = lc.cotangents(c.model, c.N, c.B, name)
    assert sum(v is not None for v in cot.values()) == 1
    shapes = lc.cotangents(c.model, c.N, c.B, "all")
    full = {k: (cot[k] if cot[k] is not None else np.zeros_like(shapes[k])) for k in shapes}
    alone, flat, zeros = c.vjp(cot), c.vjp(cot, squeeze=True), c.vjp(full)
    assert flat["x0"].shape == (c.B, c.nx) and flat["x_ref"].shape == (c.B, c.nx * c.N)
    for key in ("x0", "x_ref", "status"):
        assert np.array_equal(alone[key], zeros[key]), key
        assert np.array_equal(alone[key] if key == "status" else alone[key][:, 0], flat[key]), key
    assert np.isfinite(alone["x0"]).all() and np.isfinite(alone["x_ref"]).all()


# ---- negative statuses -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model", [0, 1])
def test_a_failed_forward_gives_status_minus_2_and_exact_zeros(fm, torch_, track, model):
    c = _case(fm, torch_, track, model, lc.N_ROWS, infeasible=True)
    bad = np.zeros(c.B, dtype=bool)
    bad[list(lc.INFEASIBLE)] = True
    assert (c.f["exitflag"][bad] != 0).all() and (c.f["exitflag"][~bad] == 0).all(), c.f["exitflag"]
    for name in ("all_k3", "fbar"):
        got, ref, sel, fig = _compare(c, name, tag="infeasible batch")
        assert (got["status"][bad] == -2).all() and (got["status"][~bad] >= 0).all(), fig
        assert not got["x0"][bad].any() and not got["x_ref"][bad].any()             # every column
        assert set(sel) == set(np.nonzero(~bad)[0]) and got["x0"][~bad].any(axis=(1, 2)).all()   # the neighbours were compared above


# ---- autograd ----------------------------------------------------------------------------------------------------------------------

def test_ltv_step_diff_gradients_with_a_slack_cotangent_equal_the_vjp(fm, torch_, track):
    torch = torch_
    c = _case(fm, torch, track, 1, lc.N_ROWS)
    cot = {k: _dev(torch, v[:, 0]) for k, v in lc.cotangents(c.model, c.N, c.B, "all").items()}
    a0, ar = c.x0.clone().requires_grad_(True), c.xr.clone().requires_grad_(True)
    status = torch.empty(c.B, dtype=torch.int32, device="cuda")
    u, x, s, f, flag, pol = fm.ltv_step_diff(c.mpc, a0, ar, c.xl, c.ul, status)
    assert torch.equal(s, c.fwd["slack"]) and torch.equal(u, c.fwd["u_opt"])
    ((u * cot["ubar"]).sum() + (x * cot["xbar"]).sum() + (s * cot["sbar"]).sum() + (f * cot["fbar"]).sum()).backward()
    ref = fm.ltv_step_vjp(c.mpc, c.fwd, c.x0, c.xr, c.xl, c.ul, **cot)
    assert torch.equal(status, ref["status"]) and (ref["status"] >= 0).sum() >= c.B * 3 // 4
    assert torch.equal(a0.grad, ref["x0"]) and torch.equal(ar.grad, ref["x_ref"])
    without = fm.ltv_step_vjp(c.mpc, c.fwd, c.x0, c.xr, c.xl, c.ul, **{k: v for k, v in cot.items() if k != "sbar"})
    assert not torch.equal(without["x0"], ref["x0"])         # the slack's cotangent does contribute
