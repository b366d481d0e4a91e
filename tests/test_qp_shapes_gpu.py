"""GPU tests of the batched QP solve (qp_prep_kernel + qp_solve_kernel / qp_wg_kernel) off the shapes the benchmark uses: LTV-MPC QPs
whose trailing 2 / 3 variables are the border (two of the four / the one 1e8-cost slack column(s) inside the MFMA core, no dummy
padding), and the generic QP families of tests/qp_families.py -- shuffled staircase rows, zero / duplicate / border-only rows, row
scales over eight decades, equality rows, a fixed variable, a zero-curvature column, nothing active at all -- at every tile count,
around the row-count thresholds of the prep kernel, with shared H and A, and in a heterogeneous batch behind the order kernel.

Every test: exit flag 0 on every instance, the numpy certificate (tests/kkt_numpy.py) <= 1e-6, the kernel's own residual <= 1e-6,
finite x, and the oracle (tests/test_qp_shapes_cpu.py shows that it meets the same conditions on the same inputs) as stated per
test.  Tolerances are those of tests/test_gpu_parity.py, nothing new.  Each test prints its figures (a line starting QPSHAPES)
before it asserts; profiles/qp_shapes/README.md records them."""
import json
import os

import numpy as np
import pytest

import qp_families as qf
from kkt_numpy import kkt_certificate
from test_gpu_parity import FVAL_TOL, KKT_TOL, X_TOL_VERTEX, _certify, _solve_dev, _vertex_agreement, _x_close
from test_qp_shapes_cpu import LTV_BORDER_SHAPES, LTV_SEED

pytestmark = pytest.mark.gpu

OUT_KEYS = ("x", "fval", "exitflag", "iter", "lam", "kkt", "polished")


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


def _oracle(orc, q):
    return orc.qp_solve_batch_aux(*[q[k] for k in qf.KEYS])


def _relx(a, b):
    return np.abs(a - b).max(axis=1) / np.maximum(1.0, np.abs(b).max(axis=1))


def _figures(group, case, q, out, ref=None, sel=None, **extra):
    """Prints the figures of one case (before anything is asserted) and returns them."""
    sel = np.arange(len(q["g"])) if sel is None else np.asarray(sel)
    qs = {k: q[k][sel] for k in qf.KEYS}
    c = kkt_certificate(*[qs[k] for k in qf.KEYS], out["x"][sel], out["lam"][sel])
    fig = dict(group=group, case=case, flags=np.unique(out["exitflag"], return_counts=True)[0].tolist(), cert=float(c["max"].max()),
               kkt=float(np.max(out["kkt"][sel])), finite=bool(np.isfinite(out["x"]).all()), refined=float((out["polished"][sel] > 0).mean()),
               iters=float(out["iter"][sel].mean()))
    if ref is not None:
        fig.update(fval_err=float(np.max(np.abs(out["fval"][sel] - ref["fval"][sel]) / np.maximum(1.0, np.abs(ref["fval"][sel])))),
                   x_err=float(_relx(out["x"][sel], ref["x"][sel]).max()), ref_refined=float((ref["polished"][sel] > 0).mean()),
                   ref_flags=np.unique(ref["exitflag"][sel]).tolist())
    fig.update(extra)
    print("QPSHAPES " + json.dumps(fig))
    return fig


def _standard(q, out, sel=None):
    """The assertions every test makes, on the instances `sel` (default: all)."""
    sel = np.arange(len(q["g"])) if sel is None else np.asarray(sel)
    assert (out["exitflag"][sel] == 0).all(), (np.nonzero(out["exitflag"] != 0)[0], out["exitflag"][out["exitflag"] != 0], out["iter"][out["exitflag"] != 0])
    assert np.isfinite(out["x"]).all()
    _certify({k: q[k][sel] for k in qf.KEYS}, {k: out[k][sel] for k in ("x", "lam")})
    assert (out["kkt"][sel] <= KKT_TOL).all(), out["kkt"][sel].max()


def _fval_close(out, ref, sel=None):
    sel = np.arange(len(ref["fval"])) if sel is None else np.asarray(sel)
    assert (ref["exitflag"][sel] == 0).all(), ref["exitflag"]
    assert (np.abs(out["fval"][sel] - ref["fval"][sel]) <= FVAL_TOL * np.maximum(1.0, np.abs(ref["fval"][sel]))).all()


# ---- 1. LTV-MPC QPs with 2- and 3-column borders --------------------------------------------------------------------------------

@pytest.mark.parametrize("model,N,B", LTV_BORDER_SHAPES)
def test_ltv_qps_with_2_and_3_column_borders(fm, torch_, orc, otrack, model, N, B):
    """Dynamic N = 7 (mod 8): nV = 2N + 4 = 2 (mod 16), kinematic N = 1 (mod 8): nV = 2N + 1 = 3 (mod 16).  qp_make_dims takes
    nV mod 16 in 1..4 as the border before it looks at the LTV signature: the NB = 4 kernels run with nb = 2 / 3 and two of the four
    (none of the one) slack columns sit inside the MFMA core -- the configuration that lost kinematic N = 20 id 15377.
    nV <= 116: one-wavefront kernel, nV = 130 / 131: workgroup kernel.  FSAEMPC_SLACK_BORDER=0 must not change which instances solve."""
    x0, xl, ul, xr = orc.synth_instances(model, N, 0.05, otrack.L, LTV_SEED, range(B))
    q = orc.build_qp_batch(model, otrack, N, 0.05, x0, xr, xl, ul)
    nV, nC = q["g"].shape[1], q["lbA"].shape[1]
    assert fm.qp_layout(nV, nC) == dict(T=nV // 16, NB=4, n_solver=nV, wavefront_kernel=nV <= 116)
    ref = _oracle(orc, q)
    out = _solve_dev(fm, torch_, q, want_aux=True)
    old_env = os.environ.get("FSAEMPC_SLACK_BORDER")
    os.environ["FSAEMPC_SLACK_BORDER"] = "0"
    try:
        off = _solve_dev(fm, torch_, q, want_aux=True)
    finally:
        if old_env is None:
            del os.environ["FSAEMPC_SLACK_BORDER"]
        else:
            os.environ["FSAEMPC_SLACK_BORDER"] = old_env
    _figures("1 ltv border", "%s N=%d nV=%d" % ("dyn" if model else "kin", N, nV), q, out, ref,
             flags_policy_on=out["exitflag"].tolist(), flags_policy_off=off["exitflag"].tolist())
    _standard(q, out)
    _fval_close(out, ref)
    _vertex_agreement(q, out, ref, (model, N))
    assert np.array_equal(off["exitflag"] == 0, out["exitflag"] == 0), (out["exitflag"], off["exitflag"])
    _standard(q, off)


# ---- 2. every tile count with nb = 2 and nb = 3 on dense data -------------------------------------------------------------------

@pytest.mark.parametrize("nV", [16 * T + nb for T in range(1, 13) for nb in (2, 3)])
def test_every_tile_count_with_border_2_and_3(fm, torch_, orc, nV):
    """nV = 16 T + 2 and 16 T + 3, T = 1..12 (T <= 7: one-wavefront kernel, else the workgroup kernel), nC = nV / 2, families R and S."""
    nC = nV // 2
    assert fm.qp_layout(nV, nC) == dict(T=nV // 16, NB=4, n_solver=nV, wavefront_kernel=nV // 16 <= 7)
    for family in ("R", "S"):
        q = qf.batch(family, nV, nC, 4)
        ref = _oracle(orc, q)
        out = _solve_dev(fm, torch_, q, want_aux=True)
        _figures("2 tile counts", "%s (%d,%d)" % (family, nV, nC), q, out, ref)
        _standard(q, out)
        _fval_close(out, ref)
        _x_close(out["x"], ref["x"], (out["polished"] > 0) & (ref["polished"] > 0), (family, nV))


# ---- 3. the families at the shape list -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("family,nV,nC", [(f, n, m) for f in qf.FAMILIES for n, m in qf.shapes(f)])
def test_families_at_the_shape_list(fm, torch_, orc, family, nV, nC):
    """F and E against their closed-form minimiser to X_TOL_VERTEX (1e-6 relative: the loosest statement the solver makes about a
    refined point; nothing is active in F, only equalities in E, so there is no flat face an interior-point iterate could sit on);
    for R and S the certificate bounds the point, fval and x are compared with the oracle as everywhere.  Measured worst error
    against x_star: 3.9e-14 (F), 4.0e-9 (E); worst certificate 1.7e-12 (F), 4.0e-7 (E), 6.5e-8 (R), 1.1e-7 (S)."""
    q = qf.batch(family, nV, nC, 8)
    ref = _oracle(orc, q)
    out = _solve_dev(fm, torch_, q, want_aux=True)
    extra = {}
    if "x_star" in q:
        extra["x_star_err"] = float(_relx(out["x"], q["x_star"]).max())
    _figures("3 families", "%s (%d,%d)" % (family, nV, nC), q, out, ref, **extra)
    _standard(q, out)
    if "x_star" in q:
        assert extra["x_star_err"] <= X_TOL_VERTEX, _relx(out["x"], q["x_star"])
    _fval_close(out, ref)
    _x_close(out["x"], ref["x"], (out["polished"] > 0) & (ref["polished"] > 0), (family, nV, nC))


# ---- 4. nC thresholds of the prep kernel ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("nC", [1, 3, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257])
@pytest.mark.parametrize("nV", [35, 20])
def test_row_count_thresholds_of_the_prep_kernel(fm, torch_, orc, nV, nC):
    """Family R at nV = 35 (T = 2, nb = 3) and nV = 20 (T = 1, nb = 4) around Kq = 1, the trip of 16 rows, the 64-row chunks of the
    counting sort / slots of the owner layout, and the switch of the prep kernel to 1024 threads above 256 rows."""
    q = qf.batch("R", nV, nC, 4)
    ref = _oracle(orc, q)
    out = _solve_dev(fm, torch_, q, want_aux=True)
    _figures("4 nC thresholds", "R (%d,%d)" % (nV, nC), q, out, ref)
    _standard(q, out)
    _fval_close(out, ref)
    _x_close(out["x"], ref["x"], (out["polished"] > 0) & (ref["polished"] > 0), (nV, nC))


# ---- 5. shared_HA ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nV,nC", [(52, 70), (130, 65)])
def test_shared_HA_is_bit_identical_to_stacked(fm, torch_, nV, nC):
    """fsaempc_qp_desc.shared_HA on the device entry: one (H, A) of family R, six different g, bounds and ranges (each around its
    own feasible point) -- every output bit-identical to the solve with H and A stacked per instance."""
    torch = torch_
    qps = [qf.make("R", nV, nC, i, ha_inst=0) for i in range(6)]
    q, qs = qf.stack(qps), qf.stack(qps, shared_HA=True)
    assert qs["H"].shape == (nV, nV) and qs["A"].shape == (nV, nC) and len(np.unique(q["g"][:, 0])) == 6
    a = _solve_dev(fm, torch, q, want_aux=True)
    b = _solve_dev(fm, torch, qs, want_aux=True, shared_HA=True)
    _figures("5 shared_HA", "stacked (%d,%d)" % (nV, nC), q, a)
    _figures("5 shared_HA", "shared (%d,%d)" % (nV, nC), q, b)
    for k in OUT_KEYS:
        assert np.array_equal(a[k], b[k]), k
    _standard(q, b)


# ---- 6. heterogeneous batch behind the order kernel ----------------------------------------------------------------------------

def test_heterogeneous_batch_matches_solo_solves(fm, torch_, orc):
    """B = 300 > 256 at (52, 70): the order kernel is active.  Instances cycle through R, S and E; one is infeasible (a duplicate row
    pair with disjoint ranges), one has a NaN in g.  Every feasible instance meets the standard assertions, the infeasible one returns
    a flag != 0 with finite x, the NaN one -1 after 0 iterations with finite x, and a solo solve (B = 1) of instances 0, 1, 150, 299
    and of both neighbours of each bad instance is bit-identical in every output."""
    nV, nC, B, i_inf, i_nan = 52, 70, 300, 100, 200
    qps = [qf.make("RSE"[i % 3], nV, nC, i) for i in range(B)]
    qps[i_inf] = qf.make_infeasible(nV, nC, i_inf)
    qps[i_nan]["g"][5] = np.nan
    q = qf.stack(qps)
    good = np.setdiff1d(np.arange(B), [i_inf, i_nan])
    out = _solve_dev(fm, torch_, q, want_aux=True)
    qg = {k: q[k][good] for k in qf.KEYS}
    refg = _oracle(orc, qg)
    ref = {k: np.zeros((B,) + v.shape[1:], dtype=v.dtype) for k, v in refg.items()}
    for k in ref:
        ref[k][good] = refg[k]
    _figures("6 heterogeneous", "RSE (52,70) x 300", q, out, ref, sel=good, bad_flags=out["exitflag"][[i_inf, i_nan]].tolist(),
             bad_iters=out["iter"][[i_inf, i_nan]].tolist())
    _standard(q, out, good)
    _fval_close(out, ref, good)
    _x_close(out["x"][good], ref["x"][good], (out["polished"][good] > 0) & (ref["polished"][good] > 0), "heterogeneous")
    assert out["exitflag"][i_inf] != 0 and np.isfinite(out["x"][i_inf]).all(), out["exitflag"][i_inf]
    assert out["exitflag"][i_nan] == -1 and out["iter"][i_nan] == 0 and np.isfinite(out["x"][i_nan]).all(), (out["exitflag"][i_nan], out["iter"][i_nan])
    for i in (0, 1, 150, 299, i_inf - 1, i_inf + 1, i_nan - 1, i_nan + 1):
        solo = _solve_dev(fm, torch_, {k: q[k][i:i + 1] for k in qf.KEYS}, want_aux=True)
        for k in OUT_KEYS:
            assert np.array_equal(solo[k][0], out[k][i]), (i, k)
