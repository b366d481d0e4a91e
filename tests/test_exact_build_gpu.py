"""The exact NLP build (SqpBatch.build_qp: ltv_build_kernel<NX, true, false, PAR>, four kernels, three integrators) against the
long-double dual-number restatement of tests/dual_numpy.py, tensor by tensor, at ragged shapes and at the largest horizon the ABI
takes; and the plain build (LtvBatch.build_qp) against the oracle at the same ragged shapes.

Tolerance per tensor: max(32 e64, 1e-13) of the tensor's max-norm, e64 being the gap of the float64 run of the same restatement to
the long-double one on the same inputs, the largest over the case's instances (tests/exact_cases.py; below 4e-13 everywhere, below
3e-14 for everything but `const`, whose residual aff - x_ref cancels).

Measured on the MI355X (largest relative error over all cases of this file, GPU against long double; DESIGN.md 6e-1 has the table
per shape): pred 1.2e-15, Bd 2.1e-15, Bt 1.1e-14, A 6.6e-15, lbA 9.2e-15, ubA 1.1e-14, lb and ub 0, H 1.8e-14, g 6.8e-16, const
3.1e-13; at most 0.25 of the tolerance (const), 0.06 for the others.  Before the exact kinematic RK4 build with compiled-in
constants was routed through its RtPar sibling (ltv_build_launch) this test failed for it at N = 3, 9, 17 with NaN in Bd."""
import numpy as np
import pytest

import dual_numpy as dn
import exact_cases as ec
from conftest import relerr

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


@pytest.fixture(scope="module")
def reference():
    """The long-double QPs and e64 per (model, N, integ, params): pure Python, computed once per case."""
    return ec.reference


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


@pytest.mark.parametrize("case", ec.exact_cases(), ids=ec.case_id)
def test_exact_build_matches_long_double(fm, torch_, reference, case):
    torch = torch_
    model, N, integ, par = case
    ref = reference(*case)
    B = ref["x0"].shape[0]
    tr = fm.Track.load(ec.TRACK)
    sb = fm.SqpBatch(model, N, ec.DT, tr, B, integrator=integ, params=ref["P"])
    q = sb.build_qp(_dev(torch, ref["x0"]), _dev(torch, ref["x_ref"]), _dev(torch, ref["u"]))
    torch.cuda.synchronize()
    q = {k: v.cpu().numpy() for k, v in q.items()}
    nx = ref["x0"].shape[1]
    bad = []
    for b in range(B):
        ld = ref["ld"][b]
        # the diagonal blocks of Bt are Bd_k itself: step and column of the worst entry
        Phi = q["Bt"][b][:2 * N].reshape(N, 2, N, nx)
        Bd = np.stack([Phi[k, :, k, :].T for k in range(N)])                      # (N, nx, 2)
        err = np.max(np.abs(Bd - ld["Bd"]), axis=1) / float(np.max(np.abs(ld["Bd"])))
        k, c = np.unravel_index(np.argmax(err), err.shape)
        tol = float(ec.tolerance(ref["e64"]["Bd"].max()))
        print("%-24s b=%d %-5s err %.2e  e64 %.2e  tol %.2e  (step %d, column %d)" % (ec.case_id(case), b, "Bd", err.max(), ref["e64"]["Bd"].max(), tol, k + 1, c))
        if not err.max() <= tol:
            bad.append(("Bd", b, "step %d column %d" % (k + 1, c), float(err.max()), tol))
        for name in ec.TENSORS:
            e = dn.gap(q[name][b], ld[name])      # (asserts the infinite and +-1e10 filler pattern)
            tol = float(ec.tolerance(ref["e64"][name].max()))
            print("%-24s b=%d %-5s err %.2e  e64 %.2e  tol %.2e" % (ec.case_id(case), b, name, e, ref["e64"][name].max(), tol))
            if not e <= tol:
                bad.append((name, b, e, tol))
    assert not bad, bad


@pytest.mark.parametrize("model", [0, 1])
@pytest.mark.parametrize("N", ec.N_SMALL)
@pytest.mark.parametrize("par", [False, True], ids=["fixed", "par"])
def test_plain_build_at_ragged_shapes(fm, torch_, orc, model, N, par):
    """The four plain kernels (LtvBatch.build_qp, default integrators) at the shapes where the SYRK's tiles are ragged, against the
    oracle at the 1e-9 of test_construction_parity.  The oracle knows the reference's constants only, so the kernels with a
    parameter block get the default block per instance."""
    torch = torch_
    B = ec.B_SMALL
    tr = fm.Track.load(ec.TRACK); otr = orc.Track.load(fm.tracks._HERE + "/tracks/%s.json" % ec.TRACK)
    x0, xl, ul, xr = fm.instances(model, N, ec.DT, tr.L, 20190, range(B))
    rng = np.random.default_rng(40 + N)
    ul = np.stack([rng.uniform(-2, 2, (B, N)), rng.uniform(-0.08, 0.08, (B, N))], axis=2)
    P = np.repeat(fm.default_params(model)[None], B, 0) if par else None
    q = fm.LtvBatch(model, N, ec.DT, tr, B, params=P).build_qp(_dev(torch, x0), _dev(torch, xr), _dev(torch, xl), _dev(torch, ul))
    torch.cuda.synchronize()
    ref = orc.build_qp_batch(model, otr, N, ec.DT, x0, xr, xl, ul, keep_prediction=True)
    for k in ("H", "g", "A", "lb", "ub", "lbA", "ubA", "const", "Bt"):
        assert relerr(q[k].cpu().numpy(), ref[k]) <= 1e-9, k
    pred = np.einsum("bcr,bc->br", ref["A_bar"], x0) + ref["d_bar"]
    assert relerr(q["pred"].cpu().numpy(), pred) <= 1e-9
