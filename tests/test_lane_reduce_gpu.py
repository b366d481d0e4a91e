"""The cross-lane reductions of the one-wavefront solve kernel (csrc/qp_lane.h: grp16_* over a DPP row, single and batched,
q_* over the four rows, wave_*): lane moves that leave the destination's old value undefined, and independent reductions done step
by step as one batch.  What can go wrong is a call site that is not convergent (a disabled lane then contributes garbage instead of
a zero), a tree that pairs other lanes than before, or a batch that mixes up its members.  The device self test compares the
primitives bit for bit; the solves below reach every code path that uses them, at the smallest shape that does:
  * dynamic N = 6 / N = 14 with the last general row removed (nV 16 / 32: no border): T = 1 (no K > 0 sums at all) and T = 2;
  * kinematic N = 8: T = 1 with a one-column border;  dynamic N = 7: T = 1 behind the widest border (nV 18);
  * kinematic N = 40: <5,1>, the headline instantiation;  dynamic N = 40: <5,4>, four border columns (batched border sums);
  * kinematic N = 56: T = 7, the tightest register budget.
On these batches (seed 20190, ids 0..B-1) the CPU oracle returns flag 0 for every instance, so no instance is left out.
Tolerances against the oracle: those of test_gpu_parity.py::test_solve_parity_generic_mode."""
import numpy as np
import pytest
from test_gpu_parity import FVAL_TOL, X_TOL, X_TOL_MED, X_TOL_P90, _solve_dev, _vertex_agreement

pytestmark = pytest.mark.gpu

# (model, N, B, general rows removed, expected layout: T, NB)
SHAPES = [(1, 6, 64, 1, (1, 0)), (1, 14, 64, 1, (2, 0)), (0, 8, 64, 0, (1, 1)), (1, 7, 64, 0, (1, 4)),
          (0, 40, 64, 0, (5, 1)), (1, 40, 64, 0, (5, 4)), (0, 56, 32, 0, (7, 1))]
IDS = ["dynN6-1row", "dynN14-1row", "kinN8", "dynN7", "kinN40", "dynN40", "kinN56"]
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


def _case(fm, torch, orc, model, N, B, drop):
    """QP batch, the oracle's solution and one solve on the GPU: computed once per shape, shared by the tests, left unchanged."""
    key = (model, N, B, drop)
    if key not in _CASES:
        otr = orc.Track.load(fm.tracks._HERE + "/tracks/fsg2019.json")
        x0, xl, ul, xr = fm.instances(model, N, 0.05, otr.L, 20190, range(B))
        q = orc.build_qp_batch(model, otr, N, 0.05, x0, xr, xl, ul)
        q = {k: q[k] for k in ("H", "g", "A", "lb", "ub", "lbA", "ubA")}
        if drop:   # A is (B, nV, nC): one column of it per general row
            q["A"] = np.ascontiguousarray(q["A"][:, :, :-drop])
            q["lbA"] = np.ascontiguousarray(q["lbA"][:, :-drop])
            q["ubA"] = np.ascontiguousarray(q["ubA"][:, :-drop])
        ref = orc.qp_solve_batch_aux(q["H"], q["g"], q["A"], q["lb"], q["ub"], q["lbA"], q["ubA"])
        _CASES[key] = (q, ref, _solve_dev(fm, torch, q, want_aux=True))
    return _CASES[key]


def test_lane_reduce_selftest(fm):
    assert fm.lib().fsaempc_selftest_lane_reduce() == 0, fm.lib().fsaempc_last_error()


@pytest.mark.parametrize("model,N,B,drop,layout", SHAPES, ids=IDS)
def test_solve_matches_the_oracle(fm, torch_, orc, model, N, B, drop, layout):
    q, ref, out = _case(fm, torch_, orc, model, N, B, drop)
    nV, nC = q["g"].shape[1], q["lbA"].shape[1]
    lay = fm.qp_layout(nV, nC)
    print("shape", (model, N, B, drop), "nV", nV, "nC", nC, "layout", lay)
    assert lay["wavefront_kernel"] and (lay["T"], lay["NB"]) == layout, lay
    fo = ref["fval"]
    ex = np.abs(out["x"] - ref["x"]).max(axis=1) / np.maximum(1, np.abs(ref["x"]).max(axis=1))
    print("flags", np.unique(out["exitflag"], return_counts=True), "oracle flags", np.unique(ref["exitflag"], return_counts=True),
          "fval err %.3e" % np.max(np.abs(out["fval"] - fo) / np.maximum(1, np.abs(fo))),
          "x err max %.3e p90 %.3e median %.3e" % (ex.max(), np.percentile(ex, 90), np.median(ex)))
    assert (ref["exitflag"] == 0).all(), np.unique(ref["exitflag"], return_counts=True)
    assert (out["exitflag"] == 0).all(), np.unique(out["exitflag"], return_counts=True)
    assert np.max(np.abs(out["fval"] - fo) / np.maximum(1, np.abs(fo))) <= FVAL_TOL
    ex, both = _vertex_agreement(q, out, ref, (model, N))
    assert ex.max() <= X_TOL and np.percentile(ex, 90) <= X_TOL_P90 and np.median(ex) <= X_TOL_MED, (ex.max(), np.percentile(ex, 90), np.median(ex))


@pytest.mark.parametrize("model,N,B,drop,layout", SHAPES, ids=IDS)
def test_second_solve_is_bit_identical(fm, torch_, orc, model, N, B, drop, layout):
    """A lane move whose destination keeps an undefined old value in some lane gives whatever that register held: it changes from
    run to run."""
    q, _, out = _case(fm, torch_, orc, model, N, B, drop)
    again = _solve_dev(fm, torch_, q, want_aux=True)
    for k in BITWISE:
        assert np.array_equal(again[k], out[k], equal_nan=True), ((model, N), k)
