"""Characterisation of the refusals of the LTV build / step entry family and of the host-buffer QP paths: for every entry, every
combination of optional descriptors it takes and every malformed input, the return code and the full fsaempc_last_error() text, as
literals recorded from the library before the entries were folded onto one host path (EXPECTED at the end of the file).  Every
refusal here happens on the host before the first HIP call, so the test needs no GPU; the buffers are host memory filled with a
sentinel that a refused call must leave alone."""
import ctypes as C
import itertools

import numpy as np
import pytest

DT, N0, B0, SENT = 0.05, 6, 3, 7.0
SEED, BLOCKED = 31, [1, 2, 3]   # the instances and the blocking tests/test_abi_paths_gpu.py compares the entries on
BUILD_OUT = ("H", "g", "A", "lb", "ub", "lbA", "ubA", "pred", "Bt", "qconst")
STEP_OUT = ("u_opt", "x_opt", "slack", "fval", "exitflag", "iter")
# entry -> (kind, slots): p parameter block, b blocking, c corridor, l lambda, a aux
ENTRIES = {
    "fsaempc_ltv_build_qp_batch_device": ("build", ""),
    "fsaempc_ltv_build_qp_batch_device_p": ("build", "p"),
    "fsaempc_ltv_build_qp_batch_device_b": ("build", "pb"),
    "fsaempc_ltv_build_qp_batch_device_c": ("build", "pbc"),
    "fsaempc_nlp_build_qp_batch_device": ("nlp", ""),
    "fsaempc_nlp_build_qp_batch_device_p": ("nlp", "p"),
    "fsaempc_ltv_step_batch_device": ("step", ""),
    "fsaempc_ltv_step_batch_device_aux": ("step", "a"),
    "fsaempc_ltv_step_batch_device_lambda": ("step", "la"),
    "fsaempc_ltv_step_batch_device_p": ("step", "pla"),
    "fsaempc_ltv_step_batch_device_b": ("step", "pbla"),
    "fsaempc_ltv_step_batch_device_c": ("step", "pbcla"),
}


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _ref(s):
    return None if s is None else C.byref(s)


class Call:
    """One call of `entry` on well-formed arguments (N = 6, batch 3); a case damages it, a mode adds the optional descriptors."""

    def __init__(self, fm, model, entry):
        from fsae_mpc_amd import _lib
        self.lib, self.L, self.entry, self.model = _lib, fm.lib(), entry, model
        self.kind, self.slots = ENTRIES[entry]
        nx, ns, nV, nC = fm.dims(model, N0)
        self.desc = _lib.LtvDesc(model, N0, B0, DT, -1)
        self.table = np.zeros(64)
        self.sp = _lib.Spline(16, 1.0, _ptr(self.table), _ptr(self.table))
        self.par = self.blk = self.cor = None
        self.auto_blk = True
        f = lambda n: np.full(B0 * n, SENT)
        self.buf = {"x0": f(nx), "x_ref": f(nx * N0), "u_lin": f(2 * N0)}
        if self.kind != "nlp":
            self.buf["x_lin"] = f(nx * N0)
        self.ins = tuple(k for k in ("x0", "x_ref", "x_lin", "u_lin") if k in self.buf)
        if self.kind == "step":
            self.buf.update(u_opt=f(2 * N0), x_opt=f(nx * N0), slack=f(ns), fval=f(1), exitflag=np.full(B0, 7, dtype=np.int32),
                            iter=np.full(B0, 7, dtype=np.int32))
            self.buf["lambda"] = f(nV + nC)
            need = self.L.fsaempc_ltv_workspace_bytes(C.byref(self.desc))
            self.buf["workspace"] = np.full(need // 8 + 1, SENT)
            self.wsb = self.buf["workspace"].size * 8
        else:
            for k, n in zip(BUILD_OUT, (nV * nV, nV, nC * nV, nV, nV, nC, nC, nx * N0, nx * N0 * nV, 1)):
                self.buf[k] = f(n)
        self.arrays = dict(self.buf)   # (a case may null an entry of buf; the array itself stays to be looked at)
        self._keep = []

    def blocking(self, lens, null_len=False):
        arr = (C.c_int * max(1, len(lens)))(*lens)
        self._keep.append(arr)
        self.blk = self.lib.LtvBlocking(len(lens), None if null_len else C.cast(arr, C.POINTER(C.c_int)))
        self.auto_blk = False

    def corridor(self, lo=True, hi=True, N_w=4, ds=1.0):
        self.cor = self.lib.CorridorTable(_ptr(self.table) if lo else None, _ptr(self.table) if hi else None, N_w, ds, 0)

    def mode(self, m):
        """m: letters of p (a shared parameter block), b (blocking [1, 2, 3]; two blocks where a case changed N), t (the trivial
        blocking), c (a well-formed corridor)."""
        N = self.desc.N if self.desc is not None else N0
        if "p" in m:
            self.values = np.full(32, 1.0)
            self.par = self.lib.LtvParams(_ptr(self.values), 0)
        if "b" in m and self.auto_blk:
            self.blocking([1, 2, 3] if N <= N0 else [N - N // 2, N // 2])
        if "t" in m and self.auto_blk:
            self.blocking([1] * max(N, 1))
        if "c" in m and self.cor is None:
            self.corridor()

    def run(self):
        a = [_ref(self.desc), _ref(self.sp)]
        for s, v in (("p", self.par), ("b", self.blk), ("c", self.cor)):
            if s in self.slots:
                a.append(_ref(v))
        a += [_ptr(self.buf[k]) for k in self.ins]
        if self.kind == "step":
            a.append(None)   # default options
            a += [_ptr(self.buf[k]) for k in STEP_OUT]
            if "l" in self.slots:
                a.append(_ptr(self.buf["lambda"]))
            if "a" in self.slots:
                a.append(None)
            a += [_ptr(self.buf["workspace"]), C.c_longlong(self.wsb)]
        else:
            a += [_ptr(self.buf[k]) for k in BUILD_OUT]
        a.append(None)   # stream
        rc = getattr(self.L, self.entry)(*a)
        msg = self.L.fsaempc_last_error().decode() if rc != 0 else ""
        clean = all(bool((v == (7 if v.dtype == np.int32 else SENT)).all()) for v in self.arrays.values())
        return rc, msg, clean


def _desc(field, value):
    return lambda c: setattr(c.desc, field, value)


def _null(name):
    return lambda c: c.buf.__setitem__(name, None)


def _both(*fs):
    return lambda c: [f(c) for f in fs]


# name -> (damage, slots the entry must have, kinds it applies to)
ALL = ("build", "nlp", "step")
CASES = {
    "desc NULL": (lambda c: setattr(c, "desc", None), "", ALL),
    "sp NULL": (lambda c: setattr(c, "sp", None), "", ALL),
    "sp->xP NULL": (lambda c: setattr(c.sp, "xP", None), "", ALL),
    "sp->yP NULL": (lambda c: setattr(c.sp, "yP", None), "", ALL),
    "sp->M = 0": (lambda c: setattr(c.sp, "M", 0), "", ALL),
    "unknown model": (_desc("model", 7), "", ALL),
    "N = 0": (_desc("N", 0), "", ALL),
    "dt = 0": (_desc("dt", 0.0), "", ALL),
    "batch = -1": (_desc("batch", -1), "", ALL),
    "integrator = 3": (_desc("integrator", 3), "", ALL),
    "integrator = -2": (_desc("integrator", -2), "", ALL),
    "batch = 0": (_desc("batch", 0), "", ALL),
    "lambda NULL": (_null("lambda"), "l", ("step",), "fsaempc_ltv_step_batch_device_lambda"),   # (optional everywhere else)
    "workspace one byte short": (lambda c: setattr(c, "wsb", c.need() - 1), "", ("step",)),
    "blocking NULL": (lambda c: setattr(c, "auto_blk", False), "b", ALL, "fsaempc_ltv_build_qp_batch_device_b", "fsaempc_ltv_step_batch_device_b"),
    "blocking: a zero length": (lambda c: c.blocking([3, 0, 3]), "b", ALL),
    "blocking: wrong sum": (lambda c: c.blocking([1, 2, 2]), "b", ALL),
    "blocking: n_blocks > N": (lambda c: c.blocking([1] * 7), "b", ALL),
    "blocking: n_blocks = 0": (lambda c: c.blocking([]), "b", ALL),
    "blocking: len NULL": (lambda c: c.blocking([1, 2, 3], null_len=True), "b", ALL),
    "corridor: n_lo NULL": (lambda c: c.corridor(lo=False), "c", ALL),
    "corridor: n_hi NULL": (lambda c: c.corridor(hi=False), "c", ALL),
    "corridor: N_w = 1": (lambda c: c.corridor(N_w=1), "c", ALL),
    "corridor: ds = 0": (lambda c: c.corridor(ds=0.0), "c", ALL),
    "corridor: ds = -1": (lambda c: c.corridor(ds=-1.0), "c", ALL),
    "corridor: ds = nan": (lambda c: c.corridor(ds=float("nan")), "c", ALL),
    "corridor: ds = inf": (lambda c: c.corridor(ds=float("inf")), "c", ALL),
    "corridor and pred NULL": (_both(lambda c: c.corridor(), _null("pred")), "c", ("build",)),
    # two defects at once: the one reported pins the order of the checks
    "bad corridor + bad blocking": (_both(lambda c: c.corridor(N_w=1), lambda c: c.blocking([3, 0, 3])), "bc", ALL),
    "bad corridor + desc NULL": (_both(lambda c: c.corridor(ds=0.0), lambda c: setattr(c, "desc", None)), "c", ALL),
    "bad blocking + x0 NULL": (_both(lambda c: c.blocking([1, 2, 2]), _null("x0")), "b", ALL),
    "bad blocking + unknown model": (_both(lambda c: c.blocking([1, 2, 2]), _desc("model", 7)), "b", ALL),
    "bad blocking + dt = 0": (_both(lambda c: c.blocking([3, 0, 3]), _desc("dt", 0.0)), "b", ALL),
    "x0 NULL + dt = 0": (_both(_null("x0"), _desc("dt", 0.0)), "", ALL),
    "x0 NULL + batch = 0": (_both(_null("x0"), _desc("batch", 0)), "", ALL),
    "workspace short + batch = 0": (_both(lambda c: setattr(c, "wsb", 0), _desc("batch", 0)), "", ("step",)),
}
for _k in ("x0", "x_ref", "x_lin", "u_lin"):
    CASES[_k + " NULL"] = (_null(_k), "", ("build", "step") if _k == "x_lin" else ALL)
for _k in ("H", "g", "A", "lb", "ub", "lbA", "ubA", "Bt"):
    CASES[_k + " NULL"] = (_null(_k), "", ("build", "nlp"))
for _k in STEP_OUT + ("workspace",):
    CASES[_k + " NULL"] = (_null(_k), "", ("step",))
# Long horizons: 2N + ns > FSAEMPC_MAX_NV from N = 98; the LDS staging ends at N = 157 for the exact build of the dynamic model,
# at 166 for its LTV build, at 296 for the kinematic LTV build with a parameter block and at 297 without.  Not every entry refuses
# them (the unblocked build has no FSAEMPC_MAX_NV check: its LDS staging is its limit), and a call that is not refused would
# launch on host pointers: EXPECTED lists those combinations with code None and the test leaves them out.
for _n in (98, 160, 297, 300):
    CASES["N = %d" % _n] = (_desc("N", _n), "", ALL)
    CASES["N = %d + x0 NULL" % _n] = (_both(_desc("N", _n), _null("x0")), "", ALL)
    CASES["N = %d + workspace NULL" % _n] = (_both(_desc("N", _n), _null("workspace")), "", ("step",))


def _need(c):
    """What the step's workspace check compares with: the blocked size where the call takes the blocked path."""
    if c.blk is not None and c.blk.n_blocks != c.desc.N:
        return c.L.fsaempc_ltv_workspace_bytes_b(C.byref(c.desc), C.byref(c.blk))
    return c.L.fsaempc_ltv_workspace_bytes(C.byref(c.desc))


Call.need = _need


def modes(slots):
    blk = ("",) if "b" not in slots else ("", "b", "t") if "c" in slots else ("b", "t")   # (a _b entry is for a blocking: see "blocking NULL")
    return ["".join(m) for m in itertools.product(("", "p") if "p" in slots else ("",), blk, ("", "c") if "c" in slots else ("",))]


def combos(cases):
    for entry, (kind, slots) in ENTRIES.items():
        for name, (_f, needs, kinds, *only) in cases.items():
            if kind in kinds and all(s in slots for s in needs) and (not only or entry in only):
                for m in modes(slots):
                    for model in (0, 1):
                        yield name, entry, m, model


def run_case(fm, cases, name, entry, m, model):
    c = Call(fm, model, entry)
    damage = cases[name][0]
    if name.startswith("workspace one byte short"):   # (the size depends on the mode's blocking: damage after the mode)
        c.mode(m)
        damage(c)
    else:
        damage(c)
        c.mode(m)
    return c.run()


def key(entry, m, model):
    return "%s %s/%s" % (entry.replace("fsaempc_", "").replace("_batch_device", ""), m or "-", "kd"[model])


def lookup(name, k):
    """EXPECTED[name]: [(rc, text, keys)], keys a list of `entry mode/model` or "*" for every combination not listed."""
    rows = EXPECTED[name]
    for rc, text, keys in rows:
        if keys != "*" and k in keys:
            return rc, text
    return [(rc, text) for rc, text, keys in rows if keys == "*"][0]


def test_every_refusal_of_the_ltv_build_and_step_entries():
    import fsae_mpc_amd as fm
    n = 0
    for name, entry, m, model in combos(CASES):
        want = lookup(name, key(entry, m, model))
        if want[0] is None:   # not refused: it would launch
            continue
        rc, msg, clean = run_case(fm, CASES, name, entry, m, model)
        assert (rc, msg) == want, (name, key(entry, m, model), rc, msg, want)
        assert clean, (name, key(entry, m, model), "a refused call wrote to a buffer")
        assert rc < 0 or "batch = 0" in name, (name, key(entry, m, model))
        n += 1
    assert n > 2000, n


def test_workspace_sizes_are_what_they_were():
    import fsae_mpc_amd as fm
    from fsae_mpc_amd import _lib
    L = fm.lib()
    got = {}
    for model, N, B in itertools.product((0, 1), (6, 40), (1, 3)):
        d = _lib.LtvDesc(model, N, B, DT, -1)
        row = [L.fsaempc_ltv_workspace_bytes(C.byref(d)), L.fsaempc_ltv_step_vjp_workspace_bytes(C.byref(d), 1),
               L.fsaempc_ltv_step_vjp_workspace_bytes(C.byref(d), 3)]
        for lens in ([1, 2, 3], [1] * 6, [2] * (N // 2), [1] * N):
            arr = (C.c_int * len(lens))(*lens)
            blk = _lib.LtvBlocking(len(lens), C.cast(arr, C.POINTER(C.c_int)))
            row.append(L.fsaempc_ltv_workspace_bytes_b(C.byref(d), C.byref(blk)))
        got[(model, N, B)] = row
        assert row[-1] == row[0]   # the trivial blocking is the unblocked step
    assert got == WORKSPACE_BYTES, got
    d = _lib.LtvDesc(0, 6, 3, DT, -1)
    assert L.fsaempc_ltv_workspace_bytes(None) == -1 and L.fsaempc_ltv_workspace_bytes_b(None, None) == -1
    assert L.fsaempc_ltv_workspace_bytes_b(C.byref(d), None) == -1 and L.fsaempc_ltv_step_vjp_workspace_bytes(C.byref(d), 0) == -1
    for bad, rc in ((dict(N=0), -1), (dict(batch=-1), -1), (dict(N=98), -2)):
        d = _lib.LtvDesc(0, 6, 3, DT, -1)
        for k, v in bad.items():
            setattr(d, k, v)
        arr = (C.c_int * 2)(d.N - d.N // 2, d.N // 2)
        blk = _lib.LtvBlocking(2, C.cast(arr, C.POINTER(C.c_int)))
        assert L.fsaempc_ltv_workspace_bytes(C.byref(d)) == rc and L.fsaempc_ltv_step_vjp_workspace_bytes(C.byref(d), 1) == rc, bad
        assert L.fsaempc_ltv_workspace_bytes_b(C.byref(d), C.byref(blk)) == rc, bad


QP_SHAPES = ((9, 0), (13, 36), (81, 240), (124, 1200), (196, 0))
LINE_SHAPES = ((1, 8), (3, 8), (2, 40), (1, 196))             # (n_plans, N_c)
CELLS_SHAPES = ((1, 16, 8), (3, 80, 40), (1, 392, 196), (1, 2048, 196))   # (n_plans, N_s, N_c)


def other_workspace_sizes(L, _lib):
    """Every size query outside the LTV step family, negative codes included: entry -> {shape: size, or sizes over the last argument}."""
    got = {"sqp": {}, "qp_s": {}, "qp_vjp": {}, "raceline": {}, "minlap": {}, "cells": {}}
    for model, N, B in itertools.product((0, 1), (6, 40), (1, 3)):
        got["sqp"][(model, N, B)] = L.fsaempc_sqp_workspace_bytes(C.byref(_lib.LtvDesc(model, N, B, DT, -1)))
    for (nV, nC), B, shared in itertools.product(QP_SHAPES, (1, 3), (0, 1)):
        d = _lib.QpDesc(nV, nC, B, shared)
        got["qp_s"][(nV, nC, B, shared)] = [L.fsaempc_qp_workspace_bytes_s(C.byref(d), s) for s in (-1, 0, 1, 4)]
        got["qp_vjp"][(nV, nC, B, shared)] = L.fsaempc_qp_vjp_workspace_bytes(C.byref(d))
    for k in LINE_SHAPES:
        got["raceline"][k] = L.fsaempc_plan_raceline_workspace_bytes(*k)
        got["minlap"][k] = [L.fsaempc_plan_minlap_workspace_bytes(*k, n_rho) for n_rho in (1, 8, 16)]
    for k in CELLS_SHAPES:
        got["cells"][k] = L.fsaempc_plan_raceline_cells_workspace_bytes(*k)
    return got


def test_the_other_workspace_sizes_are_what_they_were():
    """The SQP, the plain QP solve (every slack hint), the QP VJP and the three racing-line workspaces: the sizes the library
    reported before the C ABI glue was split into units and its layouts were written over one allocator."""
    import fsae_mpc_amd as fm
    from fsae_mpc_amd import _lib
    got = other_workspace_sizes(fm.lib(), _lib)
    for entry, want in OTHER_WORKSPACE_BYTES.items():
        assert got[entry] == want, (entry, got[entry])
    assert set(got) == set(OTHER_WORKSPACE_BYTES)


def test_the_instances_of_the_gpu_comparison_solve_on_the_oracle(orc, otrack):
    """tests/test_abi_paths_gpu.py compares entries bit for bit and asserts exit flag 0 everywhere: these are cars the oracle solves,
    unblocked and blocked, so a batch of failures cannot pass there as "equal"."""
    import block_numpy as bn
    qp = ("H", "g", "A", "lb", "ub", "lbA", "ubA")
    for model in (0, 1):
        x0, xl, ul, xr = orc.synth_instances(model, N0, DT, otrack.L, SEED, range(B0))
        q = orc.build_qp_batch(model, otrack, N0, DT, x0, xr, xl, ul)
        assert (orc.qp_solve_batch_aux(*[q[k] for k in qp])["exitflag"] == 0).all(), model
        qb = bn.block_qp(q, bn.blocking_matrix(BLOCKED, 1 if model == 0 else 4))
        assert (orc.qp_solve_batch_aux(*[qb[k] for k in qp])["exitflag"] == 0).all(), model


# ---- the host-buffer QP paths ----
QP_ARGS = ("H", "g", "A", "lb", "ub", "lbA", "ubA")
NAN_TEXT = {"H": "ERROR (qpOASES): Argument 1 contains 'NaN' or 'Inf' !", "g": "ERROR (qpOASES): Argument 2 contains 'NaN' or 'Inf' !",
            "A": "ERROR (qpOASES): Argument 3 contains 'NaN' or 'Inf' !", "lb": "ERROR (qpOASES): bounds contain 'NaN' !",
            "ub": "ERROR (qpOASES): bounds contain 'NaN' !", "lbA": "ERROR (qpOASES): constraint bounds contain 'NaN' !",
            "ubA": "ERROR (qpOASES): constraint bounds contain 'NaN' !"}
BAD_HANDLE = "ERROR (qpOASES): Invalid handle to QP instance!"


def _qp(nV=2, nC=1, B=2):
    q = dict(H=np.tile(np.eye(nV).ravel(), B), g=np.zeros(B * nV), A=np.ones(B * nC * nV), lb=-np.ones(B * nV), ub=np.ones(B * nV),
             lbA=-np.ones(B * nC), ubA=np.ones(B * nC))
    out = dict(x=np.full(B * nV, SENT), fval=np.full(B, SENT), exitflag=np.full(B, 7, dtype=np.int32), iter=np.full(B, 7, dtype=np.int32),
               lam=np.full(B * (nV + nC), SENT))
    return q, out


def _clean(out):
    return all(bool((v == (7 if v.dtype == np.int32 else SENT)).all()) for v in out.values())


def test_host_qp_solve_refusals():
    import fsae_mpc_amd as fm
    from fsae_mpc_amd import _lib
    L = fm.lib()

    def solve(desc, q, out):
        rc = L.fsaempc_qp_solve_batch(_ref(desc), *[_ptr(q[k]) for k in QP_ARGS], None, *[_ptr(out[k]) for k in ("x", "fval", "exitflag", "iter", "lam")])
        return rc, (L.fsaempc_last_error().decode() if rc else ""), _clean(out)

    for name in QP_ARGS:
        for bad in (np.nan, np.inf, -np.inf):
            if name in ("lb", "ub", "lbA", "ubA") and np.isinf(bad):
                continue   # an infinite bound is a bound that is not there, not an error
            q, out = _qp()
            q[name][-1] = bad
            assert solve(_lib.QpDesc(2, 1, 2, 0), q, out) == (-1, NAN_TEXT[name], True), (name, bad)
    # the first bad argument is the one reported
    q, out = _qp()
    q["ubA"][0] = q["lb"][1] = q["A"][0] = np.nan
    assert solve(_lib.QpDesc(2, 1, 2, 0), q, out) == (-1, NAN_TEXT["A"], True)
    q, out = _qp()
    q["ubA"][0] = q["ub"][1] = np.nan
    assert solve(_lib.QpDesc(2, 1, 2, 0), q, out) == (-1, NAN_TEXT["ub"], True)
    # with shared matrices only the first instance's H and A exist
    q, out = _qp()
    q["H"][4] = np.nan
    assert solve(_lib.QpDesc(2, 1, 2, 0), q, out) == (-1, NAN_TEXT["H"], True)
    q["g"][0] = np.inf
    assert solve(_lib.QpDesc(2, 1, 2, 1), q, out) == (-1, NAN_TEXT["g"], True)
    for name in ("H", "g", "lb", "ub"):
        q, out = _qp()
        q[name] = None
        assert solve(_lib.QpDesc(2, 1, 2, 0), q, out) == (-1, "null argument", True), name
    q, out = _qp()
    assert solve(None, q, out) == (-1, "null argument", True)
    rc = L.fsaempc_qp_solve_batch(C.byref(_lib.QpDesc(2, 1, 2, 0)), *[_ptr(q[k]) for k in QP_ARGS], None, None, None, None, None, None)
    assert (rc, L.fsaempc_last_error().decode()) == (-1, "null argument")   # x
    for name in ("A", "lbA", "ubA"):
        q, out = _qp()
        q[name] = None
        assert solve(_lib.QpDesc(2, 1, 2, 0), q, out) == (-1, "nC > 0 needs A, lbA, ubA", True), name
    q, out = _qp()
    for d in (_lib.QpDesc(0, 1, 2, 0), _lib.QpDesc(2, -1, 2, 0), _lib.QpDesc(2, 1, -1, 0)):
        assert solve(d, q, out) == (-1, "bad dimensions", True)
    assert solve(_lib.QpDesc(197, 1, 2, 0), q, out) == (-2, "nV exceeds FSAEMPC_MAX_NV", True)
    q["g"][0] = np.nan
    assert solve(_lib.QpDesc(2, 1, 0, 0), q, out) == (0, "", True)   # an empty batch: nothing is read, nothing is written


def test_sequence_entries_refuse_before_the_device_is_needed():
    """(A NaN in g or in a bound of 'i', and everything of 'h' on a live handle, is found after the matrices went to the device:
    tests/test_abi_paths_gpu.py has those.)"""
    import fsae_mpc_amd as fm
    L = fm.lib()
    err = lambda: L.fsaempc_last_error().decode()
    q, out = _qp(B=1)
    res = [_ptr(out[k]) for k in ("x", "fval", "exitflag", "iter", "lam")]
    vec = [_ptr(q[k]) for k in ("g", "lb", "ub", "lbA", "ubA")]
    h = C.c_int(99)

    def init(nV=2, nC=1, k=1, H=q["H"], A=q["A"], handle=h):
        return L.fsaempc_seq_init(nV, nC, _ptr(H), vec[0], _ptr(A), *vec[1:], k, None, _ref(handle), *res)

    for name in ("H", "A"):
        for bad in (np.nan, np.inf):
            m = q[name].copy()
            m[-1] = bad
            assert init(**{name: m}) == -1 and err() == NAN_TEXT[name] and h.value == 0 and _clean(out), (name, bad)
            h.value = 99
    for kw in (dict(handle=None), dict(H=None), dict(A=None), dict(nV=0), dict(nC=-1), dict(k=0)):
        assert init(**kw) == -1 and err() == "ERROR (qpOASES): invalid arguments to 'i'" and h.value == 99, kw
    assert init(nV=197) == -2 and err() == "nV exceeds FSAEMPC_MAX_NV" and h.value == 99
    # the four entries that take a handle
    for handle in (0, 7, -1):
        assert L.fsaempc_seq_hotstart(handle, 2, 1, *vec, 1, None, *res) == -1 and err() == BAD_HANDLE
        assert L.fsaempc_seq_hotstart_matrices(handle, 2, 1, _ptr(q["H"]), vec[0], _ptr(q["A"]), *vec[1:], 1, None, *res) == -1 and err() == BAD_HANDLE
        assert L.fsaempc_seq_equality(handle, 2, 1, *vec, 1, None, res[0], res[4], None, None) == -1 and err() == BAD_HANDLE
        assert L.fsaempc_seq_cleanup(handle) == -1 and err() == BAD_HANDLE
    assert _clean(out)


# ---- recorded from the library as it was before the change ----
WORKSPACE_BYTES = {(0, 6, 1): [44800, 20480, 22016, 41472, 44800, 41472, 44800],
 (0, 6, 3): [133120, 59136, 64000, 123392, 133120, 123392, 133120],
 (0, 40, 1): [659968, 592128, 602368, -1, -1, 354304, 659968],
 (0, 40, 3): [1978880, 1774592, 1805568, -1, -1, 1062144, 1978880],
 (1, 6, 1): [84224, 44288, 48640, 75776, 84224, 75776, 84224],
 (1, 6, 3): [251904, 131584, 144640, 226048, 251904, 226048, 251904],
 (1, 40, 1): [1590272, 1100288, 1128704, -1, -1, 934656, 1590272],
 (1, 40, 3): [4770048, 3299840, 3384832, -1, -1, 2803200, 4770048]}
OTHER_WORKSPACE_BYTES = {
 'cells': {(1, 16, 8): 33024, (1, 392, 196): 2151360, (1, 2048, 196): 7646208, (3, 80, 40): 350720},
 'minlap': {(1, 8): [38336, 169600, 319872], (1, 196): [-2, -2, -2], (2, 40): [205312, 880256, 1651840], (3, 8): [113216, 507520, 958336]},
 'qp_s': {(9, 0, 1, 0): [18432, 18432, 19456, 19456], (9, 0, 1, 1): [18432, 18432, 19456, 19456],
          (9, 0, 3, 0): [55296, 55296, 58368, 58368], (9, 0, 3, 1): [55296, 55296, 58368, 58368],
          (13, 36, 1, 0): [34816, 34816, 35840, 35840], (13, 36, 1, 1): [34816, 34816, 35840, 35840],
          (13, 36, 3, 0): [104448, 104448, 107520, 107520], (13, 36, 3, 1): [104448, 104448, 107520, 107520],
          (81, 240, 1, 0): [313856, 379392, 313856, 313856], (81, 240, 1, 1): [313856, 379392, 313856, 313856],
          (81, 240, 3, 0): [941568, 1138176, 941568, 941568], (81, 240, 3, 1): [941568, 1138176, 941568, 941568],
          (124, 1200, 1, 0): [1721344, 1710080, 1721344, 1721344], (124, 1200, 1, 1): [1721344, 1710080, 1721344, 1721344],
          (124, 1200, 3, 0): [5164032, 5130240, 5164032, 5164032], (124, 1200, 3, 1): [5164032, 5130240, 5164032, 5164032],
          (196, 0, 1, 0): [510464, -2, -2, 510464], (196, 0, 1, 1): [510464, -2, -2, 510464],
          (196, 0, 3, 0): [1531392, -2, -2, 1531392], (196, 0, 3, 1): [1531392, -2, -2, 1531392]},
 'qp_vjp': {(9, 0, 1, 0): 6400, (9, 0, 1, 1): 6400, (9, 0, 3, 0): 19200, (9, 0, 3, 1): 19200,
            (13, 36, 1, 0): 6656, (13, 36, 1, 1): 6656, (13, 36, 3, 0): 19968, (13, 36, 3, 1): 19968,
            (81, 240, 1, 0): 222976, (81, 240, 1, 1): 222976, (81, 240, 3, 0): 668928, (81, 240, 3, 1): 668928,
            (124, 1200, 1, 0): 399104, (124, 1200, 1, 1): 399104, (124, 1200, 3, 0): 1197312, (124, 1200, 3, 1): 1197312,
            (196, 0, 1, 0): 1388032, (196, 0, 1, 1): 1388032, (196, 0, 3, 0): 4164096, (196, 0, 3, 1): 4164096},
 'raceline': {(1, 8): 19264, (1, 196): -2, (2, 40): 108032, (3, 8): 56512},
 'sqp': {(0, 6, 1): 46336, (0, 6, 3): 136448, (0, 40, 1): 666112, (0, 40, 3): 1996032,
         (1, 6, 1): 86528, (1, 6, 3): 257792, (1, 40, 1): 1601536, (1, 40, 3): 4802816}}
EXPECTED = {'A NULL': [(-1, 'null argument (Bt is required as scratch)', '*')],
 'Bt NULL': [(-1, 'null argument (Bt is required as scratch)', '*')],
 'H NULL': [(-1, 'null argument (Bt is required as scratch)', '*')],
 'N = 0': [(-1, 'bad dimensions', '*')],
 'N = 160': [(-2, '2N + ns exceeds FSAEMPC_MAX_NV', '*'),
             (-2, 'nV exceeds FSAEMPC_MAX_NV',
              ['ltv_step -/k', 'ltv_step -/d', 'ltv_step_aux -/k', 'ltv_step_aux -/d', 'ltv_step_lambda -/k', 'ltv_step_lambda -/d', 'ltv_step_p -/k',
               'ltv_step_p -/d', 'ltv_step_p p/k', 'ltv_step_p p/d', 'ltv_step_c -/k', 'ltv_step_c -/d', 'ltv_step_c c/k', 'ltv_step_c c/d',
               'ltv_step_c p/k', 'ltv_step_c p/d', 'ltv_step_c pc/k', 'ltv_step_c pc/d']),
             (None, 'not refused',
              ['ltv_build_qp -/k', 'ltv_build_qp -/d', 'ltv_build_qp_p -/k', 'ltv_build_qp_p -/d', 'ltv_build_qp_p p/k', 'ltv_build_qp_p p/d',
               'ltv_build_qp_c -/k', 'ltv_build_qp_c -/d', 'ltv_build_qp_c c/k', 'ltv_build_qp_c c/d', 'ltv_build_qp_c p/k', 'ltv_build_qp_c p/d',
               'ltv_build_qp_c pc/k', 'ltv_build_qp_c pc/d', 'nlp_build_qp -/k', 'nlp_build_qp_p -/k', 'nlp_build_qp_p p/k']),
             (-2, 'horizon too long for the LDS staging', ['nlp_build_qp -/d', 'nlp_build_qp_p -/d', 'nlp_build_qp_p p/d'])],
 'N = 160 + workspace NULL': [(-2, '2N + ns exceeds FSAEMPC_MAX_NV', '*'),
                              (-1, 'null argument',
                               ['ltv_step -/k', 'ltv_step -/d', 'ltv_step_aux -/k', 'ltv_step_aux -/d', 'ltv_step_lambda -/k', 'ltv_step_lambda -/d',
                                'ltv_step_p -/k', 'ltv_step_p -/d', 'ltv_step_p p/k', 'ltv_step_p p/d', 'ltv_step_c -/k', 'ltv_step_c -/d',
                                'ltv_step_c c/k', 'ltv_step_c c/d', 'ltv_step_c p/k', 'ltv_step_c p/d', 'ltv_step_c pc/k', 'ltv_step_c pc/d'])],
 'N = 160 + x0 NULL': [(-2, '2N + ns exceeds FSAEMPC_MAX_NV', '*'),
                       (-1, 'null argument',
                        ['ltv_step -/k', 'ltv_step -/d', 'ltv_step_aux -/k', 'ltv_step_aux -/d', 'ltv_step_lambda -/k', 'ltv_step_lambda -/d',
                         'ltv_step_p -/k', 'ltv_step_p -/d', 'ltv_step_p p/k', 'ltv_step_p p/d', 'ltv_step_c -/k', 'ltv_step_c -/d', 'ltv_step_c c/k',
                         'ltv_step_c c/d', 'ltv_step_c p/k', 'ltv_step_c p/d', 'ltv_step_c pc/k', 'ltv_step_c pc/d']),
                       (-1, 'null argument (Bt is required as scratch)',
                        ['ltv_build_qp -/k', 'ltv_build_qp -/d', 'ltv_build_qp_p -/k', 'ltv_build_qp_p -/d', 'ltv_build_qp_p p/k',
                         'ltv_build_qp_p p/d', 'ltv_build_qp_c -/k', 'ltv_build_qp_c -/d', 'ltv_build_qp_c c/k', 'ltv_build_qp_c c/d',
                         'ltv_build_qp_c p/k', 'ltv_build_qp_c p/d', 'ltv_build_qp_c pc/k', 'ltv_build_qp_c pc/d', 'nlp_build_qp -/k',
                         'nlp_build_qp_p -/k', 'nlp_build_qp_p p/k']),
                       (-2, 'horizon too long for the LDS staging', ['nlp_build_qp -/d', 'nlp_build_qp_p -/d', 'nlp_build_qp_p p/d'])],
 'N = 297': [(-2, '2N + ns exceeds FSAEMPC_MAX_NV', '*'),
             (-2, 'horizon too long for the LDS staging',
              ['ltv_build_qp -/d', 'ltv_build_qp_p -/d', 'ltv_build_qp_p p/k', 'ltv_build_qp_p p/d', 'ltv_build_qp_c -/d', 'ltv_build_qp_c c/d',
               'ltv_build_qp_c p/k', 'ltv_build_qp_c p/d', 'ltv_build_qp_c pc/k', 'ltv_build_qp_c pc/d', 'nlp_build_qp -/k', 'nlp_build_qp -/d',
               'nlp_build_qp_p -/k', 'nlp_build_qp_p -/d', 'nlp_build_qp_p p/k', 'nlp_build_qp_p p/d', 'ltv_step -/d', 'ltv_step_aux -/d',
               'ltv_step_lambda -/d', 'ltv_step_p -/d', 'ltv_step_p p/d', 'ltv_step_c -/d', 'ltv_step_c c/d', 'ltv_step_c p/d', 'ltv_step_c pc/d']),
             (-2, 'nV exceeds FSAEMPC_MAX_NV',
              ['ltv_step -/k', 'ltv_step_aux -/k', 'ltv_step_lambda -/k', 'ltv_step_p -/k', 'ltv_step_p p/k', 'ltv_step_c -/k', 'ltv_step_c c/k',
               'ltv_step_c p/k', 'ltv_step_c pc/k']),
             (None, 'not refused', ['ltv_build_qp -/k', 'ltv_build_qp_p -/k', 'ltv_build_qp_c -/k', 'ltv_build_qp_c c/k'])],
 'N = 297 + workspace NULL': [(-2, '2N + ns exceeds FSAEMPC_MAX_NV', '*'),
                              (-1, 'null argument',
                               ['ltv_step -/k', 'ltv_step_aux -/k', 'ltv_step_lambda -/k', 'ltv_step_p -/k', 'ltv_step_p p/k', 'ltv_step_c -/k',
                                'ltv_step_c c/k', 'ltv_step_c p/k', 'ltv_step_c pc/k']),
                              (-2, 'horizon too long for the LDS staging',
                               ['ltv_step -/d', 'ltv_step_aux -/d', 'ltv_step_lambda -/d', 'ltv_step_p -/d', 'ltv_step_p p/d', 'ltv_step_c -/d',
                                'ltv_step_c c/d', 'ltv_step_c p/d', 'ltv_step_c pc/d'])],
 'N = 297 + x0 NULL': [(-2, '2N + ns exceeds FSAEMPC_MAX_NV', '*'),
                       (-2, 'horizon too long for the LDS staging',
                        ['ltv_build_qp -/d', 'ltv_build_qp_p -/d', 'ltv_build_qp_p p/d', 'ltv_build_qp_c -/d', 'ltv_build_qp_c c/d',
                         'ltv_build_qp_c p/d', 'ltv_build_qp_c pc/d', 'nlp_build_qp -/k', 'nlp_build_qp -/d', 'nlp_build_qp_p -/k',
                         'nlp_build_qp_p -/d', 'nlp_build_qp_p p/k', 'nlp_build_qp_p p/d', 'ltv_step -/d', 'ltv_step_aux -/d', 'ltv_step_lambda -/d',
                         'ltv_step_p -/d', 'ltv_step_p p/d', 'ltv_step_c -/d', 'ltv_step_c c/d', 'ltv_step_c p/d', 'ltv_step_c pc/d']),
                       (-1, 'null argument',
                        ['ltv_step -/k', 'ltv_step_aux -/k', 'ltv_step_lambda -/k', 'ltv_step_p -/k', 'ltv_step_p p/k', 'ltv_step_c -/k',
                         'ltv_step_c c/k', 'ltv_step_c p/k', 'ltv_step_c pc/k']),
                       (-1, 'null argument (Bt is required as scratch)',
                        ['ltv_build_qp -/k', 'ltv_build_qp_p -/k', 'ltv_build_qp_p p/k', 'ltv_build_qp_c -/k', 'ltv_build_qp_c c/k',
                         'ltv_build_qp_c p/k', 'ltv_build_qp_c pc/k'])],
 'N = 300': [(-2, '2N + ns exceeds FSAEMPC_MAX_NV', '*'),
             (-2, 'horizon too long for the LDS staging',
              ['ltv_build_qp -/k', 'ltv_build_qp -/d', 'ltv_build_qp_p -/k', 'ltv_build_qp_p -/d', 'ltv_build_qp_p p/k', 'ltv_build_qp_p p/d',
               'ltv_build_qp_c -/k', 'ltv_build_qp_c -/d', 'ltv_build_qp_c c/k', 'ltv_build_qp_c c/d', 'ltv_build_qp_c p/k', 'ltv_build_qp_c p/d',
               'ltv_build_qp_c pc/k', 'ltv_build_qp_c pc/d', 'nlp_build_qp -/k', 'nlp_build_qp -/d', 'nlp_build_qp_p -/k', 'nlp_build_qp_p -/d',
               'nlp_build_qp_p p/k', 'nlp_build_qp_p p/d', 'ltv_step -/k', 'ltv_step -/d', 'ltv_step_aux -/k', 'ltv_step_aux -/d',
               'ltv_step_lambda -/k', 'ltv_step_lambda -/d', 'ltv_step_p -/k', 'ltv_step_p -/d', 'ltv_step_p p/k', 'ltv_step_p p/d', 'ltv_step_c -/k',
               'ltv_step_c -/d', 'ltv_step_c c/k', 'ltv_step_c c/d', 'ltv_step_c p/k', 'ltv_step_c p/d', 'ltv_step_c pc/k', 'ltv_step_c pc/d'])],
 'N = 300 + workspace NULL': [(-2, '2N + ns exceeds FSAEMPC_MAX_NV', '*'),
                              (-2, 'horizon too long for the LDS staging',
                               ['ltv_step -/k', 'ltv_step -/d', 'ltv_step_aux -/k', 'ltv_step_aux -/d', 'ltv_step_lambda -/k', 'ltv_step_lambda -/d',
                                'ltv_step_p -/k', 'ltv_step_p -/d', 'ltv_step_p p/k', 'ltv_step_p p/d', 'ltv_step_c -/k', 'ltv_step_c -/d',
                                'ltv_step_c c/k', 'ltv_step_c c/d', 'ltv_step_c p/k', 'ltv_step_c p/d', 'ltv_step_c pc/k', 'ltv_step_c pc/d'])],
 'N = 300 + x0 NULL': [(-2, '2N + ns exceeds FSAEMPC_MAX_NV', '*'),
                       (-2, 'horizon too long for the LDS staging',
                        ['ltv_build_qp -/k', 'ltv_build_qp -/d', 'ltv_build_qp_p -/k', 'ltv_build_qp_p -/d', 'ltv_build_qp_p p/k',
                         'ltv_build_qp_p p/d', 'ltv_build_qp_c -/k', 'ltv_build_qp_c -/d', 'ltv_build_qp_c c/k', 'ltv_build_qp_c c/d',
                         'ltv_build_qp_c p/k', 'ltv_build_qp_c p/d', 'ltv_build_qp_c pc/k', 'ltv_build_qp_c pc/d', 'nlp_build_qp -/k',
                         'nlp_build_qp -/d', 'nlp_build_qp_p -/k', 'nlp_build_qp_p -/d', 'nlp_build_qp_p p/k', 'nlp_build_qp_p p/d', 'ltv_step -/k',
                         'ltv_step -/d', 'ltv_step_aux -/k', 'ltv_step_aux -/d', 'ltv_step_lambda -/k', 'ltv_step_lambda -/d', 'ltv_step_p -/k',
                         'ltv_step_p -/d', 'ltv_step_p p/k', 'ltv_step_p p/d', 'ltv_step_c -/k', 'ltv_step_c -/d', 'ltv_step_c c/k', 'ltv_step_c c/d',
                         'ltv_step_c p/k', 'ltv_step_c p/d', 'ltv_step_c pc/k', 'ltv_step_c pc/d'])],
 'N = 98': [(-2, '2N + ns exceeds FSAEMPC_MAX_NV', '*'),
            (None, 'not refused',
             ['ltv_build_qp -/k', 'ltv_build_qp -/d', 'ltv_build_qp_p -/k', 'ltv_build_qp_p -/d', 'ltv_build_qp_p p/k', 'ltv_build_qp_p p/d',
              'ltv_build_qp_c -/k', 'ltv_build_qp_c -/d', 'ltv_build_qp_c c/k', 'ltv_build_qp_c c/d', 'ltv_build_qp_c p/k', 'ltv_build_qp_c p/d',
              'ltv_build_qp_c pc/k', 'ltv_build_qp_c pc/d', 'nlp_build_qp -/k', 'nlp_build_qp -/d', 'nlp_build_qp_p -/k', 'nlp_build_qp_p -/d',
              'nlp_build_qp_p p/k', 'nlp_build_qp_p p/d']),
            (-2, 'nV exceeds FSAEMPC_MAX_NV',
             ['ltv_step -/k', 'ltv_step -/d', 'ltv_step_aux -/k', 'ltv_step_aux -/d', 'ltv_step_lambda -/k', 'ltv_step_lambda -/d', 'ltv_step_p -/k',
              'ltv_step_p -/d', 'ltv_step_p p/k', 'ltv_step_p p/d', 'ltv_step_c -/k', 'ltv_step_c -/d', 'ltv_step_c c/k', 'ltv_step_c c/d',
              'ltv_step_c p/k', 'ltv_step_c p/d', 'ltv_step_c pc/k', 'ltv_step_c pc/d'])],
 'N = 98 + workspace NULL': [(-2, '2N + ns exceeds FSAEMPC_MAX_NV', '*'),
                             (-1, 'null argument',
                              ['ltv_step -/k', 'ltv_step -/d', 'ltv_step_aux -/k', 'ltv_step_aux -/d', 'ltv_step_lambda -/k', 'ltv_step_lambda -/d',
                               'ltv_step_p -/k', 'ltv_step_p -/d', 'ltv_step_p p/k', 'ltv_step_p p/d', 'ltv_step_c -/k', 'ltv_step_c -/d',
                               'ltv_step_c c/k', 'ltv_step_c c/d', 'ltv_step_c p/k', 'ltv_step_c p/d', 'ltv_step_c pc/k', 'ltv_step_c pc/d'])],
 'N = 98 + x0 NULL': [(-2, '2N + ns exceeds FSAEMPC_MAX_NV', '*'),
                      (-1, 'null argument (Bt is required as scratch)',
                       ['ltv_build_qp -/k', 'ltv_build_qp -/d', 'ltv_build_qp_p -/k', 'ltv_build_qp_p -/d', 'ltv_build_qp_p p/k',
                        'ltv_build_qp_p p/d', 'ltv_build_qp_c -/k', 'ltv_build_qp_c -/d', 'ltv_build_qp_c c/k', 'ltv_build_qp_c c/d',
                        'ltv_build_qp_c p/k', 'ltv_build_qp_c p/d', 'ltv_build_qp_c pc/k', 'ltv_build_qp_c pc/d', 'nlp_build_qp -/k',
                        'nlp_build_qp -/d', 'nlp_build_qp_p -/k', 'nlp_build_qp_p -/d', 'nlp_build_qp_p p/k', 'nlp_build_qp_p p/d']),
                      (-1, 'null argument',
                       ['ltv_step -/k', 'ltv_step -/d', 'ltv_step_aux -/k', 'ltv_step_aux -/d', 'ltv_step_lambda -/k', 'ltv_step_lambda -/d',
                        'ltv_step_p -/k', 'ltv_step_p -/d', 'ltv_step_p p/k', 'ltv_step_p p/d', 'ltv_step_c -/k', 'ltv_step_c -/d', 'ltv_step_c c/k',
                        'ltv_step_c c/d', 'ltv_step_c p/k', 'ltv_step_c p/d', 'ltv_step_c pc/k', 'ltv_step_c pc/d'])],
 'bad blocking + dt = 0': [(-1, 'blocking: every block length >= 1', '*')],
 'bad blocking + unknown model': [(-1, 'blocking: the block lengths must sum to N', '*')],
 'bad blocking + x0 NULL': [(-1, 'blocking: the block lengths must sum to N', '*')],
 'bad corridor + bad blocking': [(-1, 'corridor: N_w must be >= 2', '*')],
 'bad corridor + desc NULL': [(-1, 'corridor: ds must be finite and > 0', '*')],
 'batch = -1': [(-1, 'bad dimensions', '*')],
 'batch = 0': [(0, '', '*')],
 'blocking NULL': [(-1, 'null argument', '*')],
 'blocking: a zero length': [(-1, 'blocking: every block length >= 1', '*')],
 'blocking: len NULL': [(-1, 'null argument', '*')],
 'blocking: n_blocks = 0': [(-1, 'blocking: 1 <= n_blocks <= N', '*')],
 'blocking: n_blocks > N': [(-1, 'blocking: 1 <= n_blocks <= N', '*')],
 'blocking: wrong sum': [(-1, 'blocking: the block lengths must sum to N', '*')],
 'corridor and pred NULL': [(-1, 'null argument (pred is required with a corridor)', '*')],
 'corridor: N_w = 1': [(-1, 'corridor: N_w must be >= 2', '*')],
 'corridor: ds = -1': [(-1, 'corridor: ds must be finite and > 0', '*')],
 'corridor: ds = 0': [(-1, 'corridor: ds must be finite and > 0', '*')],
 'corridor: ds = inf': [(-1, 'corridor: ds must be finite and > 0', '*')],
 'corridor: ds = nan': [(-1, 'corridor: ds must be finite and > 0', '*')],
 'corridor: n_hi NULL': [(-1, 'corridor: n_hi is NULL', '*')],
 'corridor: n_lo NULL': [(-1, 'corridor: n_lo is NULL', '*')],
 'desc NULL': [(-1, 'null argument', '*')],
 'dt = 0': [(-1, 'bad dimensions', '*')],
 'exitflag NULL': [(-1, 'null argument', '*')],
 'fval NULL': [(-1, 'null argument', '*')],
 'g NULL': [(-1, 'null argument (Bt is required as scratch)', '*')],
 'integrator = -2': [(-1, 'unknown integrator', '*')],
 'integrator = 3': [(-1, 'unknown integrator', '*')],
 'iter NULL': [(-1, 'null argument', '*')],
 'lambda NULL': [(-1, 'null argument (lambda)', '*')],
 'lb NULL': [(-1, 'null argument (Bt is required as scratch)', '*')],
 'lbA NULL': [(-1, 'null argument (Bt is required as scratch)', '*')],
 'slack NULL': [(-1, 'null argument', '*')],
 'sp NULL': [(-1, 'null argument', '*')],
 'sp->M = 0': [(-1, 'bad dimensions', '*')],
 'sp->xP NULL': [(-1, 'null argument', '*')],
 'sp->yP NULL': [(-1, 'null argument', '*')],
 'u_lin NULL': [(-1, 'null argument (Bt is required as scratch)', '*'),
                (-1, 'null argument',
                 ['ltv_step -/k', 'ltv_step -/d', 'ltv_step_aux -/k', 'ltv_step_aux -/d', 'ltv_step_lambda -/k', 'ltv_step_lambda -/d',
                  'ltv_step_p -/k', 'ltv_step_p -/d', 'ltv_step_p p/k', 'ltv_step_p p/d', 'ltv_step_b b/k', 'ltv_step_b b/d', 'ltv_step_b t/k',
                  'ltv_step_b t/d', 'ltv_step_b pb/k', 'ltv_step_b pb/d', 'ltv_step_b pt/k', 'ltv_step_b pt/d', 'ltv_step_c -/k', 'ltv_step_c -/d',
                  'ltv_step_c c/k', 'ltv_step_c c/d', 'ltv_step_c b/k', 'ltv_step_c b/d', 'ltv_step_c bc/k', 'ltv_step_c bc/d', 'ltv_step_c t/k',
                  'ltv_step_c t/d', 'ltv_step_c tc/k', 'ltv_step_c tc/d', 'ltv_step_c p/k', 'ltv_step_c p/d', 'ltv_step_c pc/k', 'ltv_step_c pc/d',
                  'ltv_step_c pb/k', 'ltv_step_c pb/d', 'ltv_step_c pbc/k', 'ltv_step_c pbc/d', 'ltv_step_c pt/k', 'ltv_step_c pt/d',
                  'ltv_step_c ptc/k', 'ltv_step_c ptc/d'])],
 'u_opt NULL': [(-1, 'null argument', '*')],
 'ub NULL': [(-1, 'null argument (Bt is required as scratch)', '*')],
 'ubA NULL': [(-1, 'null argument (Bt is required as scratch)', '*')],
 'unknown model': [(-1, 'unknown model', '*')],
 'workspace NULL': [(-1, 'null argument', '*')],
 'workspace one byte short': [(-5, 'workspace too small', '*')],
 'workspace short + batch = 0': [(0, '', '*')],
 'x0 NULL': [(-1, 'null argument (Bt is required as scratch)', '*'),
             (-1, 'null argument',
              ['ltv_step -/k', 'ltv_step -/d', 'ltv_step_aux -/k', 'ltv_step_aux -/d', 'ltv_step_lambda -/k', 'ltv_step_lambda -/d', 'ltv_step_p -/k',
               'ltv_step_p -/d', 'ltv_step_p p/k', 'ltv_step_p p/d', 'ltv_step_b b/k', 'ltv_step_b b/d', 'ltv_step_b t/k', 'ltv_step_b t/d',
               'ltv_step_b pb/k', 'ltv_step_b pb/d', 'ltv_step_b pt/k', 'ltv_step_b pt/d', 'ltv_step_c -/k', 'ltv_step_c -/d', 'ltv_step_c c/k',
               'ltv_step_c c/d', 'ltv_step_c b/k', 'ltv_step_c b/d', 'ltv_step_c bc/k', 'ltv_step_c bc/d', 'ltv_step_c t/k', 'ltv_step_c t/d',
               'ltv_step_c tc/k', 'ltv_step_c tc/d', 'ltv_step_c p/k', 'ltv_step_c p/d', 'ltv_step_c pc/k', 'ltv_step_c pc/d', 'ltv_step_c pb/k',
               'ltv_step_c pb/d', 'ltv_step_c pbc/k', 'ltv_step_c pbc/d', 'ltv_step_c pt/k', 'ltv_step_c pt/d', 'ltv_step_c ptc/k',
               'ltv_step_c ptc/d'])],
 'x0 NULL + batch = 0': [(-1, 'null argument (Bt is required as scratch)', '*'),
                         (-1, 'null argument',
                          ['ltv_step -/k', 'ltv_step -/d', 'ltv_step_aux -/k', 'ltv_step_aux -/d', 'ltv_step_lambda -/k', 'ltv_step_lambda -/d',
                           'ltv_step_p -/k', 'ltv_step_p -/d', 'ltv_step_p p/k', 'ltv_step_p p/d', 'ltv_step_b b/k', 'ltv_step_b b/d',
                           'ltv_step_b t/k', 'ltv_step_b t/d', 'ltv_step_b pb/k', 'ltv_step_b pb/d', 'ltv_step_b pt/k', 'ltv_step_b pt/d',
                           'ltv_step_c -/k', 'ltv_step_c -/d', 'ltv_step_c c/k', 'ltv_step_c c/d', 'ltv_step_c b/k', 'ltv_step_c b/d',
                           'ltv_step_c bc/k', 'ltv_step_c bc/d', 'ltv_step_c t/k', 'ltv_step_c t/d', 'ltv_step_c tc/k', 'ltv_step_c tc/d',
                           'ltv_step_c p/k', 'ltv_step_c p/d', 'ltv_step_c pc/k', 'ltv_step_c pc/d', 'ltv_step_c pb/k', 'ltv_step_c pb/d',
                           'ltv_step_c pbc/k', 'ltv_step_c pbc/d', 'ltv_step_c pt/k', 'ltv_step_c pt/d', 'ltv_step_c ptc/k', 'ltv_step_c ptc/d'])],
 'x0 NULL + dt = 0': [(-1, 'bad dimensions', '*')],
 'x_lin NULL': [(-1, 'null argument', '*'),
                (-1, 'null argument (Bt is required as scratch)',
                 ['ltv_build_qp -/k', 'ltv_build_qp -/d', 'ltv_build_qp_p -/k', 'ltv_build_qp_p -/d', 'ltv_build_qp_p p/k', 'ltv_build_qp_p p/d',
                  'ltv_build_qp_b b/k', 'ltv_build_qp_b b/d', 'ltv_build_qp_b t/k', 'ltv_build_qp_b t/d', 'ltv_build_qp_b pb/k',
                  'ltv_build_qp_b pb/d', 'ltv_build_qp_b pt/k', 'ltv_build_qp_b pt/d', 'ltv_build_qp_c -/k', 'ltv_build_qp_c -/d',
                  'ltv_build_qp_c c/k', 'ltv_build_qp_c c/d', 'ltv_build_qp_c b/k', 'ltv_build_qp_c b/d', 'ltv_build_qp_c bc/k',
                  'ltv_build_qp_c bc/d', 'ltv_build_qp_c t/k', 'ltv_build_qp_c t/d', 'ltv_build_qp_c tc/k', 'ltv_build_qp_c tc/d',
                  'ltv_build_qp_c p/k', 'ltv_build_qp_c p/d', 'ltv_build_qp_c pc/k', 'ltv_build_qp_c pc/d', 'ltv_build_qp_c pb/k',
                  'ltv_build_qp_c pb/d', 'ltv_build_qp_c pbc/k', 'ltv_build_qp_c pbc/d', 'ltv_build_qp_c pt/k', 'ltv_build_qp_c pt/d',
                  'ltv_build_qp_c ptc/k', 'ltv_build_qp_c ptc/d'])],
 'x_opt NULL': [(-1, 'null argument', '*')],
 'x_ref NULL': [(-1, 'null argument (Bt is required as scratch)', '*'),
                (-1, 'null argument',
                 ['ltv_step -/k', 'ltv_step -/d', 'ltv_step_aux -/k', 'ltv_step_aux -/d', 'ltv_step_lambda -/k', 'ltv_step_lambda -/d',
                  'ltv_step_p -/k', 'ltv_step_p -/d', 'ltv_step_p p/k', 'ltv_step_p p/d', 'ltv_step_b b/k', 'ltv_step_b b/d', 'ltv_step_b t/k',
                  'ltv_step_b t/d', 'ltv_step_b pb/k', 'ltv_step_b pb/d', 'ltv_step_b pt/k', 'ltv_step_b pt/d', 'ltv_step_c -/k', 'ltv_step_c -/d',
                  'ltv_step_c c/k', 'ltv_step_c c/d', 'ltv_step_c b/k', 'ltv_step_c b/d', 'ltv_step_c bc/k', 'ltv_step_c bc/d', 'ltv_step_c t/k',
                  'ltv_step_c t/d', 'ltv_step_c tc/k', 'ltv_step_c tc/d', 'ltv_step_c p/k', 'ltv_step_c p/d', 'ltv_step_c pc/k', 'ltv_step_c pc/d',
                  'ltv_step_c pb/k', 'ltv_step_c pb/d', 'ltv_step_c pbc/k', 'ltv_step_c pbc/d', 'ltv_step_c pt/k', 'ltv_step_c pt/d',
                  'ltv_step_c ptc/k', 'ltv_step_c ptc/d'])]}
