"""The diagonal tiles of the register Cholesky (csrc/qp_solve_kernel.h, `diag_factor`): the MFMA operand of a 4-row panel is built with
selects on constant lane masks and the diagonal tile is updated ahead of its companions; the former form stays in the source as
the reference of fsaempc_selftest_diag_factor().  The arithmetic is the same, so nothing may move: a wrong lane mask or a panel
that reads its tile too early shows up as wrong numbers (against the CPU oracle), a scheduling slip as run-to-run differences or
as a dependence on the neighbours.  Shapes:
  * kinematic N = 8 (T <= 2, border width 1), dynamic N = 7 (border width 4);
  * kinematic N = 40 at B = 300: the headline instantiation <5,1>, all five phases of pass 1, more than 256 instances so that the
    launch order is on;
  * dynamic N = 40: <5,4>;  kinematic N = 56: T = 7, the instantiation that spills.
Tolerances against the oracle: those of test_gpu_parity.py::test_solve_parity_generic_mode.  The cases (QP batch, oracle solution,
first solve) are shared with test_stream_carry_gpu.py, which solves four of the five shapes too."""
import numpy as np
import pytest
from test_gpu_parity import FVAL_TOL, X_TOL, X_TOL_MED, X_TOL_P90, _solve_dev, _vertex_agreement
from test_stream_carry_gpu import BITWISE, _case, _same_bits

pytestmark = pytest.mark.gpu

SHAPES = [(0, 8, 64), (1, 7, 64), (0, 40, 300), (1, 40, 32), (0, 56, 32)]


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


def test_diag_factor_selftest(fm):
    assert fm.lib().fsaempc_selftest_diag_factor() == 0, fm.lib().fsaempc_last_error()


@pytest.mark.parametrize("model,N,B", SHAPES)
def test_solution_matches_the_oracle(fm, torch_, orc, model, N, B):
    q, ref, out = _case(fm, torch_, orc, model, N, B, oracle=True)
    fo = ref["fval"]
    ferr = np.max(np.abs(out["fval"] - fo) / np.maximum(1, np.abs(fo)))
    ex, both = _vertex_agreement(q, out, ref, (model, N))
    print("shape", (model, N, B), "flags", np.unique(out["exitflag"], return_counts=True), "oracle flags", np.unique(ref["exitflag"], return_counts=True),
          "fval err %.3e" % ferr, "x err max %.3e p90 %.3e median %.3e" % (ex.max(), np.percentile(ex, 90), np.median(ex)))
    assert np.array_equal(out["exitflag"], ref["exitflag"]), (np.unique(out["exitflag"], return_counts=True), np.unique(ref["exitflag"], return_counts=True))
    assert ferr <= FVAL_TOL
    assert ex.max() <= X_TOL and np.percentile(ex, 90) <= X_TOL_P90 and np.median(ex) <= X_TOL_MED, (ex.max(), np.percentile(ex, 90), np.median(ex))


@pytest.mark.parametrize("model,N,B", SHAPES)
def test_second_solve_is_bit_identical(fm, torch_, orc, model, N, B):
    q, _, out = _case(fm, torch_, orc, model, N, B)
    _same_bits(_solve_dev(fm, torch_, q, want_aux=True), out, (model, N))


@pytest.mark.parametrize("model,N,B", SHAPES)
def test_reversed_batch_is_bit_identical(fm, torch_, orc, model, N, B):
    q, _, out = _case(fm, torch_, orc, model, N, B)
    rev = _solve_dev(fm, torch_, {k: v[::-1] for k, v in q.items()}, want_aux=True)
    _same_bits({k: rev[k][::-1] for k in BITWISE}, out, (model, N))
