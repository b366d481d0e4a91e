"""The thin entries of the LTV build / step family against the general (_c) one, bit for bit: each is a forward onto the same host
path with NULL for what it does not take, so both sides run the same kernels on the same inputs and every comparison is
torch.equal, never a tolerance.  The Python wrappers call the _c entries only, so the thin ones are reached through fm.lib().
Shapes: both models, fsg2019, N = 6, batch 3, the instances tests/test_abi_paths_cpu.py vets on the oracle (every exit flag is 0).
Below them: the refusals of the sequence handles that are found only after the matrices went to the device."""
import ctypes as C

import numpy as np
import pytest

from test_abi_paths_cpu import BAD_HANDLE, BLOCKED, DT, N0 as N, NAN_TEXT, B0 as B, SEED, _qp

pytestmark = pytest.mark.gpu
QP_KEYS = ("H", "g", "A", "lb", "ub", "lbA", "ubA", "pred", "Bt", "const")
STEP_KEYS = ("u_opt", "x_opt", "slack", "fval", "exitflag", "iter")


class Ctx:
    def __init__(self, model):
        import torch
        import fsae_mpc_amd as fm
        from fsae_mpc_amd import _lib
        self.torch, self.fm, self._lib, self.L, self.model = torch, fm, _lib, fm.lib(), model
        self.tr = fm.Track.load("fsg2019")
        self.nx, self.ns, self.nV, self.nC = fm.dims(model, N)
        self.mpc = fm.LtvBatch(model, N, DT, self.tr, B)   # (its spline table and descriptor serve the calls by hand too)
        self.inp = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in fm.instances(model, N, DT, self.tr.L, SEED, range(B))]
        x0, xl, ul, xr = self.inp
        self.ins = [self.p(t) for t in (x0, xr, xl, ul)]
        self.par = _lib.ParamBlock(fm.default_params(model), B, "cuda:0")
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    @staticmethod
    def p(t):
        return C.c_void_p(t.data_ptr())

    def blocking(self, lens):
        return self._lib.Blocking(lens, N)

    def build(self, suffix, *descs, nV=None):
        """fsaempc_ltv_build_qp_batch_device<suffix>(desc, sp, *descs, ...) -> the ten tensors (NaN where nothing was written)"""
        torch, nV, nC, nx = self.torch, nV or self.nV, self.nC, self.nx
        q = {k: torch.full((B * n,), float("nan"), dtype=torch.float64, device="cuda:0")
             for k, n in zip(QP_KEYS, (nV * nV, nV, nC * nV, nV, nV, nC, nC, nx * N, nx * N * nV, 1))}
        rc = getattr(self.L, "fsaempc_ltv_build_qp_batch_device" + suffix)(C.byref(self.mpc.desc), C.byref(self.mpc.sp), *descs, *self.ins,
                                                                           *[self.p(q[k]) for k in QP_KEYS], self.stream)
        assert rc == 0, (suffix, rc, self.L.fsaempc_last_error())
        torch.cuda.synchronize()
        return q

    def step(self, suffix, *descs, lam=None, aux=True, blk=None):
        """fsaempc_ltv_step_batch_device<suffix>: lam None for an entry without the argument, else True / False (NULL)"""
        torch = self.torch
        nV = self.nV if blk is None else 2 * blk.n_blocks + self.ns
        f = lambda n: torch.full((B * n,), float("nan"), dtype=torch.float64, device="cuda:0")
        out = dict(u_opt=f(2 * N), x_opt=f(self.nx * N), slack=f(self.ns), fval=f(1), exitflag=torch.full((B,), 99, dtype=torch.int32, device="cuda:0"),
                   iter=torch.full((B,), 99, dtype=torch.int32, device="cuda:0"))
        need = self.L.fsaempc_ltv_workspace_bytes_b(C.byref(self.mpc.desc), blk.ref()) if blk is not None else \
            self.L.fsaempc_ltv_workspace_bytes(C.byref(self.mpc.desc))
        assert need > 0
        ws = torch.empty((need + 7) // 8, dtype=torch.float64, device="cuda:0")
        tail = []
        if lam is not None:
            if lam:
                out["lam"] = f(nV + self.nC)
            tail.append(self.p(out["lam"]) if lam else None)
        if aux:
            tail.append(None)
        rc = getattr(self.L, "fsaempc_ltv_step_batch_device" + suffix)(C.byref(self.mpc.desc), C.byref(self.mpc.sp), *descs, *self.ins, None,
                                                                       *[self.p(out[k]) for k in STEP_KEYS], *tail, self.p(ws),
                                                                       C.c_longlong(ws.numel() * 8), self.stream)
        assert rc == 0, (suffix, rc, self.L.fsaempc_last_error())
        torch.cuda.synchronize()
        assert bool((out["exitflag"] == 0).all()), (suffix, out["exitflag"])
        return out


@pytest.fixture(scope="module", params=[0, 1], ids=["kinematic", "dynamic"])
def ctx(request):
    return Ctx(request.param)


def same(torch, a, b, keys, what):
    for k in keys:
        if k in a and k in b:
            assert torch.equal(a[k], b[k]), (what, k)
            assert not bool(torch.isnan(a[k].double()).any()), (what, k)


def test_build_entries_agree_bit_for_bit(ctx):
    t = ctx.torch
    triv, blk = ctx.blocking([1] * N), ctx.blocking(BLOCKED)
    ref = ctx.build("_c", None, None, None)
    same(t, ctx.build(""), ref, QP_KEYS, "plain")
    same(t, ctx.build("_p", None), ref, QP_KEYS, "_p(NULL)")
    same(t, ctx.build("_b", None, triv.ref()), ref, QP_KEYS, "_b(NULL, trivial)")
    par = ctx.par.ref()
    refp = ctx.build("_c", par, None, None)
    same(t, ctx.build("_p", par), refp, QP_KEYS, "_p(par)")
    same(t, ctx.build("_b", par, triv.ref()), refp, QP_KEYS, "_b(par, trivial)")
    nVb = 2 * blk.n_blocks + ctx.ns
    same(t, ctx.build("_b", None, blk.ref(), nV=nVb), ctx.build("_c", None, blk.ref(), None, nV=nVb), QP_KEYS, "_b(NULL, blocked)")


def test_step_entries_agree_bit_for_bit(ctx):
    t = ctx.torch
    triv, blk = ctx.blocking([1] * N), ctx.blocking(BLOCKED)
    keys = STEP_KEYS + ("lam",)
    ref = ctx.step("_c", None, None, None, lam=True)
    same(t, ctx.step("", aux=False), ref, keys, "plain")
    same(t, ctx.step("_aux"), ref, keys, "_aux(NULL)")
    same(t, ctx.step("_lambda", lam=True), ref, keys, "_lambda")
    same(t, ctx.step("_p", None, lam=True), ref, keys, "_p(NULL)")
    same(t, ctx.step("_p", None, lam=False), ref, keys, "_p(NULL), lambda NULL")
    same(t, ctx.step("_b", None, triv.ref(), lam=True), ref, keys, "_b(NULL, trivial)")
    same(t, ctx.step("_c", None, None, None, lam=False), ref, keys, "_c, lambda NULL")
    same(t, ctx.step("_b", None, blk.ref(), lam=True, blk=blk), ctx.step("_c", None, blk.ref(), None, lam=True, blk=blk), keys, "_b(NULL, blocked)")


def test_wrapper_is_the_general_entry(ctx):
    x0, xl, ul, xr = ctx.inp
    out = ctx.mpc.step(x0, xr, xl, ul, want_lambda=True)
    ctx.torch.cuda.synchronize()
    assert bool((out["exitflag"] == 0).all())
    ref = ctx.step("_c", None, None, None, lam=True)
    for k in STEP_KEYS + ("lam",):
        assert ctx.torch.equal(out[k].reshape(-1), ref[k]), k
    bat = ctx.fm.LtvBatch(ctx.model, N, DT, ctx.tr, B, blocking=BLOCKED, params=ctx.fm.default_params(ctx.model))
    out = bat.step(x0, xr, xl, ul, want_lambda=True)
    ctx.torch.cuda.synchronize()
    assert bool((out["exitflag"] == 0).all())
    ref = ctx.step("_c", bat.params.ref(), bat.blocking.ref(), None, lam=True, blk=bat.blocking)
    for k in STEP_KEYS + ("lam",):
        assert ctx.torch.equal(out[k].reshape(-1), ref[k]), k


def test_sequence_refusals_that_need_the_device():
    import fsae_mpc_amd as fm
    L = fm.lib()
    err = lambda: L.fsaempc_last_error().decode()
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    q, out = _qp(B=1)
    res = [ptr(out[k]) for k in ("x", "fval", "exitflag", "iter", "lam")]
    h = C.c_int(0)
    vecs = lambda d: [ptr(d[k]) for k in ("g", "lb", "ub", "lbA", "ubA")]
    init = lambda d: L.fsaempc_seq_init(2, 1, ptr(d["H"]), ptr(d["g"]), ptr(d["A"]), *vecs(d)[1:], 1, None, C.byref(h), *res)
    for name in ("g", "lb", "ub", "lbA", "ubA"):
        for bad in (np.nan,) + ((np.inf,) if name == "g" else ()):
            d = {k: v.copy() for k, v in q.items()}
            d[name][-1] = bad
            assert init(d) == -1 and err() == NAN_TEXT[name] and h.value == 0, (name, bad)
    sent = {k: v.copy() for k, v in out.items()}
    assert all(np.array_equal(out[k], sent[k]) for k in out)
    assert init(q) == 0 and h.value >= 1, err()
    assert out["exitflag"][0] == 0
    try:
        keep = {k: v.copy() for k, v in out.items()}
        for name in ("g", "lb", "ub", "lbA", "ubA"):
            d = {k: v.copy() for k, v in q.items()}
            d[name][0] = np.nan
            assert L.fsaempc_seq_hotstart(h.value, 2, 1, *vecs(d), 1, None, *res) == -1 and err() == NAN_TEXT[name], name
            assert L.fsaempc_seq_hotstart_matrices(h.value, 2, 1, ptr(d["H"]), ptr(d["g"]), ptr(d["A"]), *vecs(d)[1:], 1, None, *res) == -1
            assert err() == NAN_TEXT[name], name
        for name in ("H", "A"):
            d = {k: v.copy() for k, v in q.items()}
            d[name][0] = np.inf
            assert L.fsaempc_seq_hotstart_matrices(h.value, 2, 1, ptr(d["H"]), ptr(d["g"]), ptr(d["A"]), *vecs(d)[1:], 1, None, *res) == -1
            assert err() == NAN_TEXT[name], name
        assert L.fsaempc_seq_hotstart(h.value, 3, 1, *vecs(q), 1, None, *res) == -1
        assert err() == "ERROR (qpOASES): QP dimensions must be constant during a sequence!"
        assert L.fsaempc_seq_hotstart(h.value, 2, 1, *vecs(q), 0, None, *res) == -1 and err() == "ERROR (qpOASES): invalid arguments to 'h'"
        assert L.fsaempc_seq_hotstart(h.value, 2, 1, None, *vecs(q)[1:], 1, None, *res) == -1 and err() == "null argument"
        assert all(np.array_equal(out[k], keep[k]) for k in out)   # a refused call writes nothing
        assert L.fsaempc_seq_hotstart(h.value, 2, 1, *vecs(q), 1, None, *res) == 0 and out["exitflag"][0] == 0
    finally:
        assert L.fsaempc_seq_cleanup(h.value) == 0
    assert L.fsaempc_seq_cleanup(h.value) == -1 and err() == BAD_HANDLE
