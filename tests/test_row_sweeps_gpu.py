"""GPU tests of the row sweeps of qp_solve_kernel (row phase 2, step length, update): the sweeps load their owner-layout slots in
batches of SweepBatch<T, NB>::nsb slots (6 on the T = 5 kernels with a border, 2 elsewhere), a sweep of one trip hands its slots
to the update sweep in registers, and the variable-bound slots take their directions from the n-vectors instead of the row arrays.

The cases put the slot count JT = J + JB (J = ceil(nC / 64) slots of A rows, JB = ceil(nV / 64) slots of variable bounds) one under,
on, one over the batch and on 2 * batch + 1, at nV = 81 (T = 5, NB = 1, JB = 2: batch 6) and at nV = 20 (T = 1, NB = 4, JB = 1: the
pairwise sweep at the same row counts); nC = 64 J - 3 leaves invalid lanes in the last A slot, nC = 256 leaves none; (81, 240) is
the benchmark's shape, (84, 800) the dynamic model's (T = 5, NB = 4, 15 slots: three trips).  The rows mix two-sided, one-sided,
free (both sides infinite) and equality rows, the bounds one-sided, two-sided and one fixed variable.

Acceptance is that of tests/test_qp_shapes_gpu.py (_standard: flag 0, finite x, the numpy certificate and the kernel's residual
<= 1e-6) and agreement with the CPU oracle (fval to 1e-6, x by what both sides say they returned), same tolerances.  The oracle
returns flag 0 on every instance of every case (checked on the CPU; asserted again here)."""
import numpy as np
import pytest

import qp_families as qf
from test_gpu_parity import _solve_dev, _x_close
from test_qp_shapes_gpu import _figures, _fval_close, _oracle, _standard, fm, torch_  # noqa: F401  (fm, torch_: fixtures)

pytestmark = pytest.mark.gpu

B = 4
# (nV, nC, T, NB, slots per batch, JT)
CASES = [(81, 189, 5, 1, 6, 5), (81, 253, 5, 1, 6, 6), (81, 317, 5, 1, 6, 7), (81, 701, 5, 1, 6, 13),
         (81, 256, 5, 1, 6, 6), (81, 240, 5, 1, 6, 6), (84, 800, 5, 4, 6, 15),
         (20, 253, 1, 4, 2, 5), (20, 317, 1, 4, 2, 6), (20, 381, 1, 4, 2, 7), (20, 765, 1, 4, 2, 13)]


def mixed_rows(nV, nC, inst):
    """Family R (one- and two-sided rows over eight decades of scale, a zero row, a duplicate pair, every second upper bound infinite,
    variable 3 fixed) with every fifth row freed (both sides infinite, +-inf and the 1e10 filler in turn) and up to nV / 4 rows made
    equalities at the feasible point the family is built around."""
    q = qf.make("R", nV, nC, inst)
    xs = q["lb"] + 1.0
    xs[3] = q["lb"][3]
    ax = q["A"] @ xs
    rows = np.arange(nC)
    free = (rows >= 5) & (rows % 5 == 0)
    q["lbA"][free] = np.where(rows[free] % 2 == 0, -np.inf, -qf.FILLER)
    q["ubA"][free] = np.where(rows[free] % 2 == 0, qf.FILLER, np.inf)
    eq = rows[(rows >= 5) & (rows % 9 == 7)][: nV // 4]
    q["lbA"][eq] = ax[eq]
    q["ubA"][eq] = ax[eq]
    q["x_star"] = None
    return q


def mixed_batch(nV, nC):
    return qf.stack([mixed_rows(nV, nC, i) for i in range(B)])


@pytest.mark.parametrize("nV,nC,T,NB,nsb,JT", CASES)
def test_row_sweeps_at_the_batch_boundaries(fm, torch_, orc, nV, nC, T, NB, nsb, JT):
    lay = fm.qp_layout(nV, nC)
    assert (lay["T"], lay["NB"], lay["wavefront_kernel"]) == (T, NB, True), lay
    assert -(-nC // 64) + -(-lay["n_solver"] // 64) == JT
    q = mixed_batch(nV, nC)
    fin_l, fin_u = np.abs(q["lbA"]) < 1e9, np.abs(q["ubA"]) < 1e9
    assert (fin_l & fin_u & (q["lbA"] < q["ubA"])).any() and (fin_l ^ fin_u).any() and (~fin_l & ~fin_u).any() and (fin_l & (q["lbA"] == q["ubA"])).any()
    ref = _oracle(orc, q)
    assert (ref["exitflag"] == 0).all(), ref["exitflag"]
    out = _solve_dev(fm, torch_, q, want_aux=True)
    _figures("row sweeps", "mixed (%d,%d) JT=%d batch=%d" % (nV, nC, JT, nsb), q, out, ref)
    _standard(q, out)
    _fval_close(out, ref)
    _x_close(out["x"], ref["x"], (out["polished"] > 0) & (ref["polished"] > 0), (nV, nC))
