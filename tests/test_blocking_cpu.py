"""CPU tests of move blocking (held inputs): the numpy restatement against the oracle, the validation of a blocking,
the struct mirror, the solver's layout choice with and without the slack hint, and what the new entries do without a device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import block_numpy as bn
from kkt_numpy import kkt_certificate

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DT, SEED = 0.05, 31
# (model, N, block lengths, track, batch of the full check)
SHAPES = [
    (0, 40, [1] * 8 + [2] * 8 + [4] * 4, "fsg2019", 128),
    (0, 40, [2] * 20, "fss2019", 128),
    (1, 40, [1] * 8 + [2] * 8 + [4] * 4, "fsg2019", 128),
    (1, 80, [1] * 16 + [2] * 16 + [4] * 8, "fsg2019", 64),
    (1, 60, [1] * 12 + [2] * 12 + [4] * 6, "fss2019", 64),
    (0, 20, [1] * 4 + [2] * 4 + [4] * 2, "fsg2019", 128),
    # M = 13: two column tiles of the build's SYRK, the second beginning at step 11 -- weighted row 33, no multiple of 4 (its first
    # k-step is the floor of 33 / 4, the only batch here in which that floor rounds), with a ragged tail (3 N = 63)
    (0, 21, [1] * 5 + [2] * 8, "fsg2019", 3),
    (1, 21, [1] * 5 + [2] * 8, "fsg2019", 3),
]
QP = ("H", "g", "A", "lb", "ub", "lbA", "ubA")
NEW = ["fsaempc_ltv_blocked_nV", "fsaempc_ltv_build_qp_batch_device_b", "fsaempc_ltv_workspace_bytes_b", "fsaempc_ltv_step_batch_device_b",
       "fsaempc_qp_workspace_bytes_s", "fsaempc_qp_solve_batch_device_s", "fsaempc_qp_layout"]


@pytest.mark.parametrize("model,N,lens,track,_B", SHAPES)
def test_block_numpy_identities_on_oracle_qps(orc, track_path, model, N, lens, track, _B):
    otr = orc.Track.load(track_path(track))
    ns = 1 if model == 0 else 4
    B = 8
    assert np.array_equal(bn.blocking_matrix([1] * N, ns), np.eye(2 * N + ns))
    E = bn.blocking_matrix(lens, ns)
    assert E.shape == (2 * N + ns, 2 * len(lens) + ns) and (E.sum(axis=1) == 1).all()
    assert np.array_equal(E.sum(axis=0)[: 2 * len(lens)], np.repeat(lens, 2))
    x0, xl, ul, xr = orc.synth_instances(model, N, DT, otr.L, SEED, range(B))
    q = orc.build_qp_batch(model, otr, N, DT, x0, xr, xl, ul)
    qb = bn.block_qp(q, E)
    assert qb["H"].shape == (B, E.shape[1], E.shape[1]) and qb["A"].shape == (B, E.shape[1], q["A"].shape[2])
    full = orc.qp_solve_batch_aux(*[q[k] for k in QP])
    blk = orc.qp_solve_batch_aux(*[qb[k] for k in QP])
    assert (blk["exitflag"] == 0).all() and (full["exitflag"] == 0).all(), (blk["exitflag"], full["exitflag"])
    # a restriction of the feasible set: the blocked optimum is never below the unblocked one
    assert (blk["fval"] >= full["fval"] - 1e-9 * np.abs(full["fval"])).all(), (blk["fval"] - full["fval"])
    # the expanded blocked solution is a feasible point of the unblocked QP with the same objective
    z = blk["x"] @ E.T
    f_full = 0.5 * np.einsum("bi,bji,bj->b", z, q["H"], z) + np.einsum("bi,bi->b", q["g"], z)
    assert np.max(np.abs(f_full - blk["fval"]) / np.maximum(1.0, np.abs(blk["fval"]))) <= 1e-9
    c = kkt_certificate(*[qb[k] for k in QP], blk["x"], blk["lam"])
    assert c["max"].max() <= 1e-6, {k: float(np.max(c[k])) for k in ("stationarity", "primal", "sign", "complementarity")}


def test_blocking_validation_happens_before_the_library_is_touched():
    code = """
import sys
sys.path.insert(0, %r)
import fsae_mpc_amd as fm
for bad in ([1] * 9, [1] * 11, [5, 0, 5], [5, -1, 6], [], [2.5, 7.5]):
    try:
        fm.LtvBatch(fm.KINEMATIC, 10, 0.05, None, 4, blocking=bad)
    except ValueError:
        pass
    else:
        raise SystemExit("no ValueError for %%r" %% (bad,))
    try:
        fm.ClosedLoop(fm.KINEMATIC, 10, 0.05, None, [[0.0] * 7], blocking=bad)
    except ValueError:
        pass
    else:
        raise SystemExit("ClosedLoop: no ValueError for %%r" %% (bad,))
assert fm._lib._LIB is None, "the library was loaded"
b = fm._lib.Blocking([1, 2, 3, 4], 10)
assert b.n_blocks == 4 and b.block_of_step == [0, 1, 1, 2, 2, 2, 3, 3, 3, 3] and b.start == [0, 1, 3, 6] and not b.trivial
assert fm._lib.Blocking([1] * 10, 10).trivial
print("ok")
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)


def test_blocking_struct_matches_the_header(tmp_path):
    from fsae_mpc_amd import _lib
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fsaempc.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu\\n", sizeof(fsaempc_ltv_blocking), offsetof(fsaempc_ltv_blocking, n_blocks), '
                   'offsetof(fsaempc_ltv_blocking, len));\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    S = _lib.LtvBlocking
    assert out == [C.sizeof(S), S.n_blocks.offset, S.len.offset], out


def test_qp_layout_with_and_without_the_slack_hint():
    import fsae_mpc_amd as fm
    # reference-shaped QPs: the hint that matches changes nothing
    for nV, nC, ns in ((81, 240, 1), (124, 1200, 4), (41, 120, 1), (84, 800, 4), (164, 1600, 4)):
        assert fm.qp_layout(nV, nC) == fm.qp_layout(nV, nC, n_slack=ns), (nV, nC)
    assert fm.qp_layout(81, 240) == dict(T=5, NB=1, n_solver=81, wavefront_kernel=True)
    assert fm.qp_layout(124, 1200) == dict(T=8, NB=4, n_solver=132, wavefront_kernel=False)
    # dynamic N = 80 in 40 blocks: the signature is gone (nC != 10 (nV - 4)); NB = 4 without the hint only because 84 mod 16 = 4
    assert fm.qp_layout(84, 1600, n_slack=4) == dict(T=5, NB=4, n_solver=84, wavefront_kernel=True)
    assert fm.qp_layout(84, 1600)["NB"] == 4 and fm.qp_layout(84, 1600)["T"] == 5
    # dynamic N = 60 in 30 blocks: 64 mod 16 = 0, so without the hint the slack columns sit inside the matrix-core part
    assert fm.qp_layout(64, 1200, n_slack=4) == dict(T=4, NB=4, n_solver=68, wavefront_kernel=True)
    assert fm.qp_layout(64, 1200) == dict(T=4, NB=0, n_solver=64, wavefront_kernel=True)
    # kinematic blocked shapes of the table: nV_b = 41 and 21 (mod 16 = 9 and 5)
    assert fm.qp_layout(41, 240, n_slack=1) == dict(T=3, NB=1, n_solver=49, wavefront_kernel=True)
    assert fm.qp_layout(41, 240)["NB"] == 0
    assert fm.qp_layout(21, 120, n_slack=1) == dict(T=2, NB=1, n_solver=33, wavefront_kernel=True)
    assert fm.qp_layout(44, 800, n_slack=4) == dict(T=3, NB=4, n_solver=52, wavefront_kernel=True)
    assert fm.qp_layout(50, 10, n_slack=0) == dict(T=4, NB=0, n_solver=50, wavefront_kernel=True)
    with pytest.raises(ValueError):
        fm.qp_layout(84, 1600, n_slack=3)
    L = fm.lib()
    out = (C.c_int * 4)()
    assert L.fsaempc_qp_layout(C.byref(fm._lib.QpDesc(4, 10, 1, 0)), 4, out) == -1        # no variable left for the core
    assert L.fsaempc_qp_layout(C.byref(fm._lib.QpDesc(200, 10, 1, 0)), 4, out) == -2
    # size and solve share the hint: the padded core needs the larger workspace
    d = fm._lib.QpDesc(64, 1200, 16, 0)
    assert L.fsaempc_qp_workspace_bytes_s(C.byref(d), -1) == L.fsaempc_qp_workspace_bytes(C.byref(d))
    assert L.fsaempc_qp_workspace_bytes_s(C.byref(d), 4) > L.fsaempc_qp_workspace_bytes(C.byref(d))
    assert L.fsaempc_qp_workspace_bytes_s(C.byref(d), 2) == -1


def _blocking(lens):
    arr = (C.c_int * max(1, len(lens)))(*lens)
    from fsae_mpc_amd import _lib
    return _lib.LtvBlocking(len(lens), C.cast(arr, C.POINTER(C.c_int))), arr


def test_blocked_entries_check_their_arguments_and_compute_nothing_without_a_gpu():
    import torch
    import fsae_mpc_amd as fm
    L = fm.lib()
    for s in NEW:
        assert s in fm._lib.EXPORTS and hasattr(L, s), s
    blk, _keep = _blocking([1, 2, 3, 4])
    assert L.fsaempc_ltv_blocked_nV(fm.KINEMATIC, C.byref(blk)) == 9 and L.fsaempc_ltv_blocked_nV(fm.DYNAMIC, C.byref(blk)) == 12
    assert L.fsaempc_ltv_blocked_nV(fm.DYNAMIC, None) == -1
    tr = fm.Track.load("fsg2019")
    N, B = 10, 2
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    p = lambda a: C.c_void_p(a.data_ptr())
    xP, yP = t(tr.xP.T), t(tr.yP.T)
    sp = fm._lib.Spline(tr.M, tr.dl, C.c_void_p(xP.data_ptr()), C.c_void_p(yP.data_ptr()))
    for model in (fm.KINEMATIC, fm.DYNAMIC):
        nx, ns, nV, nC = fm.dims(model, N)
        nVb = 2 * 4 + ns
        x0, xl, ul, xr = fm.instances(model, N, DT, tr.L, SEED, range(B))
        desc = fm._lib.LtvDesc(model, N, B, DT, -1)
        outs = [torch.full((B * n,), 7.0, dtype=torch.float64) for n in (nV * nV, nV, nC * nV, nV, nV, nC, nC, nx * N, nx * N * nV, 1)]
        build = lambda d, b: L.fsaempc_ltv_build_qp_batch_device_b(C.byref(d), C.byref(sp), None, C.byref(b), p(t(x0)), p(t(xr)), p(t(xl)), p(t(ul)),
                                                                   *[p(o) for o in outs], None)
        # argument checks come first, whatever the machine
        for bad in ([1, 2, 3, 3], [1, 2, 3, 5], [5, 0, 5], [10, -1, 1], []):
            bb, _k = _blocking(bad)
            assert build(desc, bb) == -1, bad
            assert L.fsaempc_ltv_workspace_bytes_b(C.byref(desc), C.byref(bb)) == -1, bad
        long_desc = fm._lib.LtvDesc(model, 100, B, DT, -1)
        lb_, _k2 = _blocking([10] * 10)
        assert L.fsaempc_ltv_workspace_bytes_b(C.byref(long_desc), C.byref(lb_)) == -2     # 2N + ns > FSAEMPC_MAX_NV stays a dimension error
        assert all(bool((o == 7.0).all()) for o in outs)
        need = L.fsaempc_ltv_workspace_bytes_b(C.byref(desc), C.byref(blk))
        assert 0 < need < L.fsaempc_ltv_workspace_bytes(C.byref(desc))
        triv, _k3 = _blocking([1] * N)
        assert L.fsaempc_ltv_workspace_bytes_b(C.byref(desc), C.byref(triv)) == L.fsaempc_ltv_workspace_bytes(C.byref(desc))
        if torch.cuda.is_available():
            continue     # the rest states what happens without a device
        assert build(desc, blk) == -4 and all(bool((o == 7.0).all()) for o in outs)       # FSAEMPC_ERR_NODEVICE
        ws = torch.zeros(need // 8 + 1, dtype=torch.float64)
        res = [torch.full((B * n,), 7.0, dtype=torch.float64) for n in (2 * N, nx * N, ns, 1)]
        fl, it = torch.full((B,), 7, dtype=torch.int32), torch.full((B,), 7, dtype=torch.int32)
        rc = L.fsaempc_ltv_step_batch_device_b(C.byref(desc), C.byref(sp), None, C.byref(blk), p(t(x0)), p(t(xr)), p(t(xl)), p(t(ul)), None,
                                               *[p(o) for o in res], p(fl), p(it), None, None, p(ws), C.c_longlong(ws.numel() * 8), None)
        assert rc == -4 and all(bool((o == 7.0).all()) for o in res) and bool((fl == 7).all())
        qd = fm._lib.QpDesc(nVb, nC, B, 0)
        qws = torch.zeros(L.fsaempc_qp_workspace_bytes_s(C.byref(qd), ns) // 8 + 1, dtype=torch.float64)
        z = [torch.full((B * n,), 7.0, dtype=torch.float64) for n in (nVb, 1)]
        H, g, A = torch.zeros(B * nVb * nVb, dtype=torch.float64), torch.zeros(B * nVb, dtype=torch.float64), torch.zeros(B * nVb * nC, dtype=torch.float64)
        bA = torch.zeros(B * nC, dtype=torch.float64)
        rc = L.fsaempc_qp_solve_batch_device_s(C.byref(qd), ns, p(H), p(g), p(A), p(g), p(g), p(bA), p(bA), None, p(z[0]), p(z[1]), p(fl), p(it),
                                               None, None, p(qws), C.c_longlong(qws.numel() * 8), None)
        assert rc == -4 and bool((z[0] == 7.0).all()) and bool((fl == 7).all())
