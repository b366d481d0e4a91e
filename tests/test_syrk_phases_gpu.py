"""GPU tests of pass 1 of qp_solve_kernel (pass_syrk: M = H + A'DA on the matrix cores, p1..p3 beside them) at the places where its
phase structure can go wrong.  The pass walks the operand stream trip by trip (4 k-steps = 16 rows); the trips are sorted by the
number C of column tiles their rows reach, so the pass is T phases with a compile-time tile count each, and the accumulator tiles
a phase reaches are held in AGPRs across its trips.  A phase may have no trip, one trip or many, the per-row coefficients are
re-staged at every fourth trip (tr & 3 == 0), and every tile count has its own kernel.

  dense rows      every row reaches the last column tile, so only phase C = T runs: nV = 17, 33, 49, 81, 113 (T = 1, 2, 3, 5, 7, one
                  border column) times nC = 3, 16, 17, 64, 80, which is 1, 1, 2, 4, 5 trips (one under, on and one over a full trip; on
                  and one over the coefficient stage).  The QPs are family R of tests/qp_families.py with the zero tail of every row
                  filled in (R's own rows end at a random column); the all-zero row, the row on the last variable and the duplicate
                  pair stay.
  family R        the same shapes with R's own rows: a random last column per row, so the trips spread over the phases at random,
                  empty phases among them.
  staircase rows  the LTV-MPC QPs of LtvBatch.build_qp, whose rows reach one more column tile every few steps of the horizon, so
                  every phase runs: kinematic N = 8, 16, 24, 40 (T = 1, 2, 3, 5) and dynamic N = 40 ((84, 800): T = 5, four border
                  columns).

Acceptance is that of tests/test_row_sweeps_gpu.py: _standard (flag 0, finite x, the numpy certificate and the kernel's residual
<= 1e-6) and agreement with the CPU oracle (fval to 1e-6, x by what both sides say they returned), same tolerances.  The oracle
returns flag 0 on instances 0..3 of every case (checked on the CPU, asserted again here), so no instance had to be replaced."""
import numpy as np
import pytest

import qp_families as qf
from test_gpu_parity import _solve_dev, _x_close
from test_qp_shapes_gpu import _figures, _fval_close, _oracle, _standard, fm, torch_  # noqa: F401  (fm, torch_: fixtures)

pytestmark = pytest.mark.gpu

B = 4
NVS = [17, 33, 49, 81, 113]
NCS = [(3, 1), (16, 1), (17, 2), (64, 4), (80, 5)]   # (nC, trips of 16 rows)
LTV_SEED = 20190
LTV_CASES = [(0, 8), (0, 16), (0, 24), (0, 40), (1, 40)]   # (model, N); model 0 kinematic, 1 dynamic


def dense_rows(nV, nC, inst):
    """Family R with full row extent: the zero tail of every row (behind R's random last column) is filled with entries of the row's
    scale, the ranges keep their widths around the new A xs.  Rows 1 (all zero) and 2 (last variable only) stay; 4 stays a copy of 3."""
    q = qf.make("R", nV, nC, inst)
    A0 = q["A"].copy()
    xs = q["lb"] + 1.0
    xs[3] = q["lb"][3]
    rng = np.random.default_rng([20261, nV, nC, inst])
    fill = rng.standard_normal((nC, nV))
    rows = np.arange(nC)
    keep = (rows == 1) | (rows == 2)
    scale = np.where(keep, 0.0, np.abs(A0).max(axis=1))
    A = np.where(A0 != 0.0, A0, fill * scale[:, None])
    if nC > 4:
        A[4] = A[3]
    shift = (A - A0) @ xs
    q["A"] = A
    q["lbA"] = q["lbA"] + shift
    q["ubA"] = q["ubA"] + shift
    q["x_star"] = None
    return q


def generic_batch(kind, nV, nC):
    make = dense_rows if kind == "dense" else (lambda n, m, i: qf.make("R", n, m, i))
    return qf.stack([make(nV, nC, i) for i in range(B)])


def _check(kind, case, q, out, ref):
    _figures("syrk phases", "%s %s" % (kind, case), q, out, ref)
    assert (ref["exitflag"] == 0).all(), ref["exitflag"]
    _standard(q, out)
    _fval_close(out, ref)
    _x_close(out["x"], ref["x"], (out["polished"] > 0) & (ref["polished"] > 0), (kind, case))


@pytest.mark.parametrize("nC,trips", NCS)
@pytest.mark.parametrize("nV", NVS)
@pytest.mark.parametrize("kind", ["dense", "R"])
def test_generic_rows_at_every_tile_count_and_trip_count(fm, torch_, orc, kind, nV, nC, trips):
    lay = fm.qp_layout(nV, nC)
    assert (lay["T"], lay["NB"], lay["n_solver"], lay["wavefront_kernel"]) == (nV // 16, 1, nV, True), lay
    assert -(-nC // 16) == trips
    q = generic_batch(kind, nV, nC)
    if kind == "dense":   # every row but the two short ones reaches the last column tile of the core: one phase holds every trip
        reach = (np.abs(q["A"][:, 16 * (nV // 16 - 1):nV - 1, :]).max(axis=1) > 0).sum(axis=1)
        assert (reach >= nC - 2).all(), reach
    ref = _oracle(orc, q)
    out = _solve_dev(fm, torch_, q, want_aux=True)
    _check(kind, (nV, nC), q, out, ref)


@pytest.mark.parametrize("model,N", LTV_CASES)
def test_staircase_rows_of_the_ltv_qps(fm, torch_, orc, model, N):
    tr = fm.Track.load("fsg2019")
    nV, nC = (2 * N + 4, 20 * N) if model else (2 * N + 1, 6 * N)
    lay = fm.qp_layout(nV, nC)
    assert (lay["T"], lay["NB"], lay["wavefront_kernel"]) == (nV // 16, 4 if model else 1, True), lay
    x0, xl, ul, xr = fm.instances(model, N, 0.05, tr.L, LTV_SEED, range(B))
    dev = lambda a: torch_.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    qd = fm.LtvBatch(model, N, 0.05, tr, B).build_qp(dev(x0), dev(xr), dev(xl), dev(ul))
    torch_.cuda.synchronize()
    q = {k: qd[k].cpu().numpy() for k in qf.KEYS}
    assert q["g"].shape == (B, nV) and q["lbA"].shape == (B, nC)
    # the staircase: the rows' last column tiles cover every tile count 1..T, so every phase of the pass has trips
    last = np.array([np.nonzero(np.abs(q["A"][0, :16 * (nV // 16), r]) > 0)[0].max() // 16 if np.abs(q["A"][0, :16 * (nV // 16), r]).max() > 0 else -1
                     for r in range(nC)])
    assert set(range(nV // 16)) <= set(last.tolist()), sorted(set(last.tolist()))
    ref = _oracle(orc, q)
    out = _solve_dev(fm, torch_, q, want_aux=True)
    _check("ltv", ("dyn" if model else "kin", N), q, out, ref)
