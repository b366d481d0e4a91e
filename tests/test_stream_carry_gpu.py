"""The operand stream of the one-wavefront solve kernel (csrc/qp_solve_kernel.h, `Stream`): one object per kernel invocation, its
producer state lives across the passes and is restarted at the top of each (a producer carried across passes and wrapped at the end
of A~ was measured and removed: profiles/stream_carry/README.md).  What can go wrong is a record read before it has landed, or a consumer that finds another record than the one
it expects at its slot.  Either shows up as wrong numbers (against the CPU oracle), as run-to-run differences (two solves of one
batch in one process) or as a dependence on the neighbours (the batch in reversed order).  Shapes:
  * kinematic N = 2, 3, 4: fewer records than the lead of the stream (a carried producer wraps several times per pass);
  * kinematic N = 8, dynamic N = 7: T = 1..2 with border widths 1 / 4, a ring of 3..6 slots;
  * kinematic N = 40 at B = 300: the headline instantiation <5,1>, more than 256 instances so that the launch order is on;
  * dynamic N = 40: <5,4>;  kinematic N = 56: T = 7, the longest ring.
Tolerances against the oracle: those of test_gpu_parity.py::test_solve_parity_generic_mode."""
import numpy as np
import pytest
from test_gpu_parity import FVAL_TOL, X_TOL, X_TOL_MED, X_TOL_P90, _solve_dev, _vertex_agreement

pytestmark = pytest.mark.gpu

SHAPES = [(0, 2, 64), (0, 3, 64), (0, 4, 64), (0, 8, 64), (1, 7, 64), (0, 40, 300), (1, 40, 64), (0, 56, 32)]
BITWISE = ("x", "fval", "exitflag", "iter", "kkt", "polished", "lam")

_CASES = {}


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


def _case(fm, torch, orc, model, N, B, oracle=False):
    """QP batch, one solve on the GPU and (on request) the oracle's solution: computed once per shape, shared by the tests and left
    unchanged."""
    key = (model, N, B)
    if key not in _CASES:
        otr = orc.Track.load(fm.tracks._HERE + "/tracks/fsg2019.json")
        x0, xl, ul, xr = fm.instances(model, N, 0.05, otr.L, 20190, range(B))
        q = orc.build_qp_batch(model, otr, N, 0.05, x0, xr, xl, ul)
        q = {k: q[k] for k in ("H", "g", "A", "lb", "ub", "lbA", "ubA")}
        _CASES[key] = [q, None, _solve_dev(fm, torch, q, want_aux=True)]
    c = _CASES[key]
    if oracle and c[1] is None:
        c[1] = orc.qp_solve_batch_aux(c[0]["H"], c[0]["g"], c[0]["A"], c[0]["lb"], c[0]["ub"], c[0]["lbA"], c[0]["ubA"])
    return c


def _same_bits(a, b, what):
    for k in BITWISE:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k, np.nonzero(np.atleast_1d((a[k] != b[k]).reshape(len(a[k]), -1).any(axis=1)))[0][:8])


@pytest.mark.parametrize("model,N,B", SHAPES)
def test_carried_stream_matches_the_oracle(fm, torch_, orc, model, N, B):
    q, ref, out = _case(fm, torch_, orc, model, N, B, oracle=True)
    fo = ref["fval"]
    ex = np.abs(out["x"] - ref["x"]).max(axis=1) / np.maximum(1, np.abs(ref["x"]).max(axis=1))
    print("shape", (model, N, B), "flags", np.unique(out["exitflag"], return_counts=True), "oracle flags", np.unique(ref["exitflag"], return_counts=True),
          "fval err %.3e" % np.max(np.abs(out["fval"] - fo) / np.maximum(1, np.abs(fo))),
          "x err max %.3e p90 %.3e median %.3e" % (ex.max(), np.percentile(ex, 90), np.median(ex)))
    # (kinematic N = 2: the oracle itself stops one instance of the 64 at its iteration limit, flag 1 -- and so must the kernel)
    assert np.array_equal(out["exitflag"], ref["exitflag"]), (np.unique(out["exitflag"], return_counts=True), np.unique(ref["exitflag"], return_counts=True))
    assert (ref["exitflag"] == 0).mean() >= 0.95, np.unique(ref["exitflag"], return_counts=True)
    assert np.max(np.abs(out["fval"] - fo) / np.maximum(1, np.abs(fo))) <= FVAL_TOL
    ex, both = _vertex_agreement(q, out, ref, (model, N))
    assert ex.max() <= X_TOL and np.percentile(ex, 90) <= X_TOL_P90 and np.median(ex) <= X_TOL_MED, (ex.max(), np.percentile(ex, 90), np.median(ex))


@pytest.mark.parametrize("model,N,B", SHAPES)
def test_second_solve_is_bit_identical(fm, torch_, orc, model, N, B):
    """A record consumed before it has landed is a race: its outcome changes from run to run."""
    q, _, out = _case(fm, torch_, orc, model, N, B)
    _same_bits(_solve_dev(fm, torch_, q, want_aux=True), out, (model, N))


@pytest.mark.parametrize("model,N,B", SHAPES)
def test_reversed_batch_is_bit_identical(fm, torch_, orc, model, N, B):
    """Every instance owns its stream and its ring: its result does not depend on its place in the batch or on its neighbours."""
    q, _, out = _case(fm, torch_, orc, model, N, B)
    rev = _solve_dev(fm, torch_, {k: v[::-1] for k, v in q.items()}, want_aux=True)
    _same_bits({k: rev[k][::-1] for k in BITWISE}, out, (model, N))


def test_early_exits_leave_their_neighbours_alone(fm, torch_, orc):
    """Instances that never enter the iteration loop (flag -1: non-finite data, found by the prep kernel; flag -2: crossed bounds) still
    start the stream in the set-up pass and must end it cleanly; every other instance of the batch is bit-identical to the plain solve."""
    model, N, B = 0, 40, 64
    q, _, out = _case(fm, torch_, orc, model, N, B)
    p = {k: v.copy() for k, v in q.items()}
    p["g"][5, 3] = np.nan
    p["H"][40, 7, 7] = np.inf
    p["lb"][9, 0], p["ub"][9, 0] = 1.0, -1.0
    p["lbA"][63, 2], p["ubA"][63, 2] = 2.0, -2.0
    o = _solve_dev(fm, torch_, p, want_aux=True)
    fl = o["exitflag"]
    assert fl[5] == -1 and fl[40] == -1 and fl[9] == -2 and fl[63] == -2, fl[[5, 40, 9, 63]]
    assert (o["iter"][[5, 40, 9, 63]] == 0).all() and np.isfinite(o["x"]).all()
    keep = np.setdiff1d(np.arange(B), [5, 40, 9, 63])
    _same_bits({k: o[k][keep] for k in BITWISE}, {k: out[k][keep] for k in BITWISE}, "neighbours")
