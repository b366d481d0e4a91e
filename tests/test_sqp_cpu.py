"""CPU tests of the batched SQP's host side: the ctypes mirror of its structures matches include/fsaempc.h, the defaults, option
checks, and no CPU fallback without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_sqp_struct_layouts_match_the_header(tmp_path):
    from fsae_mpc_amd import _lib
    src = tmp_path / "layout.c"
    src.write_text(r"""
#include <stdio.h>
#include <stddef.h>
#include "fsaempc.h"
int main(void) {
  printf("opts %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(fsaempc_sqp_opts), offsetof(fsaempc_sqp_opts, max_sweeps),
         offsetof(fsaempc_sqp_opts, trials), offsetof(fsaempc_sqp_opts, tol_step), offsetof(fsaempc_sqp_opts, tol_feas),
         offsetof(fsaempc_sqp_opts, armijo), offsetof(fsaempc_sqp_opts, rho0), offsetof(fsaempc_sqp_opts, warm_start));
  printf("aux %zu %zu %zu %zu %zu %zu\n", sizeof(fsaempc_sqp_aux), offsetof(fsaempc_sqp_aux, lambda), offsetof(fsaempc_sqp_aux, qp_iter),
         offsetof(fsaempc_sqp_aux, step_norm), offsetof(fsaempc_sqp_aux, hard_viol), offsetof(fsaempc_sqp_aux, merit));
  return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict((l.split()[0], [int(v) for v in l.split()[1:]]) for l in subprocess.check_output([str(exe)], text=True).splitlines())
    O, A = _lib.SqpOpts, _lib.SqpAux
    assert out["opts"] == [C.sizeof(O)] + [getattr(O, f).offset for f, _ in O._fields_], out["opts"]
    assert out["aux"] == [C.sizeof(A)] + [getattr(A, f).offset for f, _ in A._fields_], out["aux"]


def test_sqp_default_opts_and_workspace():
    import fsae_mpc_amd as fm
    o = fm._lib.sqp_default_opts()
    assert (o.max_sweeps, o.trials, o.tol_step, o.tol_feas, o.armijo, o.rho0, o.warm_start) == (20, 8, 1e-6, 1e-6, 1e-4, 1.0, 1)
    with pytest.raises(TypeError):
        fm._lib.sqp_default_opts(sweeps=3)
    d = fm._lib.LtvDesc(fm.DYNAMIC, 80, 16, 0.05, -1)
    assert fm.lib().fsaempc_sqp_workspace_bytes(C.byref(d)) > fm.lib().fsaempc_ltv_workspace_bytes(C.byref(d))
    d = fm._lib.LtvDesc(fm.DYNAMIC, 100, 16, 0.05, -1)   # nV = 204 > FSAEMPC_MAX_NV
    assert fm.lib().fsaempc_sqp_workspace_bytes(C.byref(d)) == -2


def test_sqp_has_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import fsae_mpc_amd as fm
    tr = fm.Track.load("fsg2019")
    N, B = 10, 2
    x0, _, ul, xr = fm.instances(fm.KINEMATIC, N, 0.05, tr.L, 31, range(B))
    sb = fm.SqpBatch(fm.KINEMATIC, N, 0.05, tr, B, device="cpu")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    with pytest.raises(fm.FsaempcError):
        sb.solve(t(x0), t(xr), t(ul))
    with pytest.raises(fm.FsaempcError):
        sb.build_qp(t(x0), t(xr), t(ul))
