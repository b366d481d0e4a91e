"""GPU tests of the work done once per QP: qp_prep_kernel (column-run staging of the A repack, 16-byte stream stores, batched H repack)
and the start-up pass of the one-wavefront solve kernel (v = G x and A~'w of the initial multipliers in one pass over A~).

The device self test compares the start-up pass with the two passes it replaces, bit for bit.  Everything else is a solve: a wrong
element anywhere in the operand stream, the H tiles, the border columns or the bounds shows up in the numpy certificate
(tests/kkt_numpy.py), which is computed from the caller's data.  Helpers and tolerances are those of tests/test_gpu_parity.py and
tests/test_qp_shapes_gpu.py, nothing new.  Each case prints its figures (a line starting QPSHAPES) before it asserts."""
import numpy as np
import pytest

import qp_families as qf
from test_gpu_parity import _solve_dev, _x_close
from test_qp_shapes_gpu import OUT_KEYS, _figures, _fval_close, _oracle, _standard

pytestmark = pytest.mark.gpu


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


def prep_tw(np_, nC):
    """qp_make_dims' rule for the columns staged per pass of the A repack: halve from 16 while the prep kernel's LDS (the n-vector of
    column scales, 16 partial maxima, the staging tile of tw x (4 Kq + 1) doubles, the row scales; the int arrays of the sort) exceeds
    96 KiB, but never below 2.  np_: padded vector length of the shape (16 T, + 16 with a border)."""
    Kq = (nC + 3) // 4
    ntr = (Kq + 3) // 4
    tw = 16
    while True:
        lds = (np_ + 16 + tw * (4 * Kq + 1) + nC + 2) * 8 + (4 * Kq + 16 * ntr + 16 + 2 * ntr + 1 + ((nC + 63) // 64) * 16 + 6) * 4
        if lds <= 96 * 1024 or tw == 2:
            return tw
        tw >>= 1


PREP_ROWS_256_THREADS = 512   # qp_launch: the prep kernel runs on 256 threads up to this many rows, on 1024 above

# (nV, padded length np, [(nC, staging width) ...]): the last row count of every width and the first of the next
STAGING = [(20, 32, [(668, 16), (669, 8), (1196, 8), (1197, 4), (1972, 4), (1973, 2)]),
           (35, 48, [(668, 16), (669, 8), (1196, 8), (1197, 4), (1968, 4), (1969, 2)])]


def test_initial_point_selftest(fm):
    assert fm.lib().fsaempc_selftest_initial_point() == 0, fm.lib().fsaempc_last_error()


def test_staging_width_thresholds_are_those_of_the_rule():
    for nV, np_, cases in STAGING:
        for nC, tw in cases:
            assert prep_tw(np_, nC) == tw, (nV, nC)
            assert nC > PREP_ROWS_256_THREADS   # the 1024-thread launch of the prep kernel


def _solve_and_check(fm, torch_, orc, group, nV, nC):
    q = qf.batch("R", nV, nC, 4)
    ref = _oracle(orc, q)
    out = _solve_dev(fm, torch_, q, want_aux=True)
    _figures(group, "R (%d,%d)" % (nV, nC), q, out, ref)
    _standard(q, out)
    _fval_close(out, ref)
    _x_close(out["x"], ref["x"], (out["polished"] > 0) & (ref["polished"] > 0), (nV, nC))
    return q, out


@pytest.mark.parametrize("nV,nC", [(nV, nC) for nV, _, cases in STAGING for nC, _ in cases])
def test_staging_width_thresholds_of_the_prep_kernel(fm, torch_, orc, nV, nC):
    """Family R, batch 4, on both sides of every halving of the staging width (16 -> 8 -> 4 -> 2 columns per pass), nV = 20 (T = 1,
    nb = 4) and nV = 35 (T = 2, nb = 3).  The oracle refines few of these instances, so the x comparison may be empty: the
    certificate is the binding check."""
    assert fm.qp_layout(nV, nC) == dict(T=nV // 16, NB=4, n_solver=nV, wavefront_kernel=True)
    _solve_and_check(fm, torch_, orc, "startup staging", nV, nC)


@pytest.mark.parametrize("nC", [PREP_ROWS_256_THREADS, PREP_ROWS_256_THREADS + 1])
@pytest.mark.parametrize("nV", [35, 20])
def test_thread_count_switch_of_the_prep_kernel(fm, torch_, orc, nV, nC):
    """The last row count on 256 threads and the first on 1024 (sixteen columns staged per pass at both)."""
    assert prep_tw(48 if nV == 35 else 32, nC) == 16
    _solve_and_check(fm, torch_, orc, "startup prep threads", nV, nC)


@pytest.mark.parametrize("nV,nC,n_solver", [(25, 72, 33), (41, 120, 49)])
def test_dummy_padded_core_through_the_repack(fm, torch_, orc, nV, nC, n_solver):
    """The kinematic signature nC = 3 (nV - 1): the slack column is the border, the core is padded with dummy variables."""
    assert nC == 3 * (nV - 1)
    assert fm.qp_layout(nV, nC)["n_solver"] == n_solver
    _solve_and_check(fm, torch_, orc, "startup dummy core", nV, nC)


def test_headline_shape_and_solo_solve(fm, torch_, orc):
    """Family R at the headline shape (81, 240); a solo solve (B = 1) of instance 0 is bit-identical in every output to the batch."""
    q, out = _solve_and_check(fm, torch_, orc, "startup headline", 81, 240)
    solo = _solve_dev(fm, torch_, {k: q[k][0:1] for k in qf.KEYS}, want_aux=True)
    for k in OUT_KEYS:
        assert np.array_equal(solo[k][0], out[k][0]), k
