"""CPU tests of the batched SQP as the controller of the closed loop: the identities of the restatement
(tests/nmpc_loop_numpy.py) the GPU tests compare the device with, the argument checks of Nmpc and of ClosedLoop(controller=...), made
before the library is touched, and the refusals of the three new entries of the C ABI on host buffers."""
import os
import re
import subprocess
import sys

import numpy as np

import nmpc_cases as nc
import nmpc_loop_numpy as nl

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ["fsaempc_sqp_batch_device_m", "fsaempc_cl_nmpc_shift_batch_device", "fsaempc_cl_nmpc_accept_batch_device"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_new_names_exist():
    import fsae_mpc_amd as fm
    L = fm.lib()
    header = open(os.path.join(ROOT, "include", "fsaempc.h")).read()
    for s in NEW:
        assert s in fm._lib.EXPORTS and hasattr(L, s) and ("%s(" % s) in header, s
    for name in ("Nmpc", "nmpc_shift", "nmpc_accept"):
        assert name in fm.__all__ and hasattr(fm, name)
    m = re.search(r"#define\s+FSAEMPC_SQP_SKIPPED\s+(\d+)", header)
    assert m and int(m.group(1)) == fm._lib.SQP_SKIPPED == 4 and fm.sqp.STATUS[4] == "skipped"
    assert set(fm.sqp.STATUS) == set(nl.STATUSES)
    src = open(os.path.join(ROOT, "fsae-mpc_amd", "csrc", "sqp.h")).read()
    m = re.search(r"SQP_RUNNING\s*=\s*(\d+)", src)
    assert m and int(m.group(1)) == 3                      # the internal "still running" is not a status a caller sees, and not 4
    tool = open(os.path.join(ROOT, "tools", "closed_loop_bench.py")).read()
    for flag in ("--nmpc", "--nmpc-trials"):
        assert flag in tool
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert "$(LIBDIR)/cl_nmpc.o" in mk.split("COMMON :=")[1].split("\n")[0] and "$(CSRC)/cl_nmpc.h" in mk
    for f in ("cl_nmpc.h", "cl_nmpc.hip"):
        assert os.path.exists(os.path.join(ROOT, "fsae-mpc_amd", "csrc", f))


def test_shift_identities():
    rng = np.random.default_rng(1)
    for N in (1, 2, 10):
        u = rng.standard_normal((7, N, 2))
        u[3, 0, 0] = -0.0; u[4, N - 1, 1] = np.nan
        assert np.array_equal(_bits(nl.shift(u, 0)), _bits(u))                     # shift = 0 is the identity
        s = nl.shift(u, 1)
        assert np.array_equal(_bits(s[:, : N - 1]), _bits(u[:, 1:])) and np.array_equal(_bits(s[:, N - 1]), _bits(u[:, N - 1]))
        v = u
        for _ in range(N):
            v = nl.shift(v, 1)
        assert np.array_equal(_bits(v), _bits(np.repeat(u[:, N - 1:], N, axis=1)))  # N shifts: the last input everywhere
        assert np.array_equal(_bits(nl.shift(v, 1)), _bits(v))                      # ... which is a fixed point
    assert u[3, 0, 0] == 0 and np.signbit(u[3, 0, 0])                              # (the input is not written)
    assert np.array_equal(nl.skip(None, 4), np.zeros(4, dtype=np.int32))
    assert np.array_equal(nl.skip(np.array([0, 1, 2, 0, -3]), 5), np.array([0, 1, 1, 0, 1], dtype=np.int32))


def test_accept_identities():
    rng = np.random.default_rng(2)
    B, Lx, Lu = 9, 70, 20
    xn, un = rng.standard_normal((B, Lx)), rng.standard_normal((B, Lu))
    xk, uk = np.full((B, Lx), nc.SENTINEL), np.full((B, Lu), nc.SENTINEL)
    st = np.array([0, 1, 2, -1, -2, 4, 0, 1, 2], dtype=np.int32)
    it = np.arange(10, 10 + B, dtype=np.int32)
    # all finite, nobody skipped: a copy, whatever the status
    x1, u1, ef, i1 = nl.accept(xn, un, st, it, None, xk, uk)
    assert np.array_equal(_bits(x1), _bits(xn)) and np.array_equal(_bits(u1), _bits(un)) and np.array_equal(i1, it)
    assert np.array_equal(ef, [0, 0, 2, -1, -2, 4, 0, 0, 2])
    assert (xk == nc.SENTINEL).all() and (uk == nc.SENTINEL).all()                 # (the inputs are not written)
    assert np.array_equal(nl.accept(xn, un, st, None, None, xk, uk)[3], np.zeros(B, dtype=np.int32))
    # the exit-flag map over the six statuses
    assert np.array_equal(nl.exitflag(np.array(nl.STATUSES)), [0, 0, 2, -1, -2, 4])
    # one non-finite entry anywhere keeps the car's plan; a skipped car keeps it too and reports 0 / 0
    bad_x, bad_u = xn.copy(), un.copy()
    bad_x[1, 0] = np.nan; bad_x[2, 64] = np.nan; bad_u[3, Lu - 1] = np.inf; bad_x[4, Lx - 1] = -np.inf
    sk = np.zeros(B, dtype=np.int32); sk[[5, 6]] = [1, 2]
    x2, u2, ef2, i2 = nl.accept(bad_x, bad_u, st, it, sk, xk, uk)
    kept = np.array([0, 1, 1, 1, 1, 1, 1, 0, 0], dtype=bool)
    assert (x2[kept] == nc.SENTINEL).all() and (u2[kept] == nc.SENTINEL).all()
    assert np.array_equal(_bits(x2[~kept]), _bits(xn[~kept])) and np.array_equal(_bits(u2[~kept]), _bits(un[~kept]))
    assert np.array_equal(ef2, [0, 0, 2, -1, -2, 0, 0, 0, 2]) and np.array_equal(i2, np.where(sk != 0, 0, it))


def test_abi_refusals_on_host_buffers():
    """Every FSAEMPC_ERR_ARG case of the three entries is decided before any launch: with host buffers too, which stay untouched."""
    nc.check_abi_refusals("cpu")


def test_python_options_are_checked_before_the_library_is_touched():
    code = """
import sys
sys.path.insert(0, %r)
import numpy as np
import fsae_mpc_amd as fm
inf, nan = float("inf"), float("nan")
bad = [dict(sweeps=0), dict(sweeps=-1), dict(sweeps=1.5), dict(sweeps="2"), dict(sweeps=True), dict(skip_finished=1), dict(skip_finished=None),
       dict(max_sweeps=3), dict(tolerance=1e-6), dict(trials=0), dict(trials=65), dict(trials=2.0), dict(trials=True), dict(tol_step=-1e-9),
       dict(tol_step=nan), dict(tol_feas=inf), dict(tol_feas="tight"), dict(armijo=-0.1), dict(rho0=-1.0), dict(rho0=nan), dict(warm_start=2),
       dict(warm_start=0.5), dict(warm_start="on")]
for kw in bad:
    try:
        fm.Nmpc(**kw)
    except ValueError:
        continue
    raise SystemExit("no ValueError for Nmpc(%%r)" %% (kw,))
ok = fm.Nmpc()
assert ok.sweeps == 1 and ok.skip_finished is True and ok.sqp_opts == {}
ok = fm.Nmpc(sweeps=np.int64(4), skip_finished=False, trials=64, tol_step=0, tol_feas=1e-5, armijo=0.5, rho0=0.0, warm_start=False)
assert ok.sweeps == 4 and ok.skip_finished is False and ok.sqp_opts == dict(trials=64, tol_step=0.0, tol_feas=1e-5, armijo=0.5, rho0=0.0, warm_start=0)
cart = [[0.0] * 7] * 3
ctl = fm.Nmpc(sweeps=2)
refused = [(dict(controller=ctl, corridor=object()), NotImplementedError, "corridor"),
           (dict(controller=ctl, blocking=[2] * 5), NotImplementedError, "move blocking"),
           (dict(controller=ctl, warm_start=True), ValueError, "warm_start"),
           (dict(controller="nmpc"), ValueError, "Nmpc"), (dict(controller=2), ValueError, "Nmpc"), (dict(controller=dict(sweeps=2)), ValueError, "Nmpc"),
           (dict(controller=fm.Nmpc), ValueError, "Nmpc")]
for kw, exc, word in refused:
    for model in (fm.KINEMATIC, fm.DYNAMIC):
        try:
            fm.ClosedLoop(model, 10, 0.05, None, cart, **kw)
        except exc as e:
            assert type(e) is exc and word in str(e), (kw, str(e))
        else:
            raise SystemExit("no %%s for ClosedLoop(%%r)" %% (exc.__name__, kw))
for kw, exc, word in refused[1:]:
    try:
        fm.monte_carlo(fm.KINEMATIC, 10, fm.Track.load("fsg2019"), 3, 1, **kw)
    except exc as e:
        assert word in str(e), (kw, str(e))
    else:
        raise SystemExit("no %%s for monte_carlo(%%r)" %% (exc.__name__, kw))
# the texts of the two NotImplementedErrors are SqpBatch's own
for kw in (dict(corridor=object()), dict(blocking=[2] * 5)):
    texts = []
    for make in (lambda: fm.SqpBatch(fm.KINEMATIC, 10, 0.05, None, 3, **kw), lambda: fm.ClosedLoop(fm.KINEMATIC, 10, 0.05, None, cart, controller=ctl, **kw)):
        try:
            make()
        except NotImplementedError as e:
            texts.append(str(e))
    assert len(texts) == 2 and texts[0] == texts[1], texts
# a bad blocking is still a ValueError, and the trivial blocking is not refused here (it fails later, at the missing track)
try:
    fm.ClosedLoop(fm.KINEMATIC, 10, 0.05, None, cart, controller=ctl, blocking=[3] * 5)
except ValueError:
    pass
else:
    raise SystemExit("no ValueError for a blocking that does not sum to N")
assert fm._lib._LIB is None, "the library was loaded"
print("ok")
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)
