"""The cases and inputs shared by tests/test_exact_dual_cpu.py and tests/test_exact_build_gpu.py, the long-double reference QPs of
tests/dual_numpy.py on them (computed once per case and cached) and e64, the relative gap of the float64 run of the same
restatement to the long-double one: the error a correct double implementation makes, and the base of the GPU tolerance.
Also the cases of the build reproducibility tests (tests/test_build_repro_gpu.py and its child tests/build_words_child.py)."""
import functools
import os

import numpy as np

import dual_numpy as dn

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TRACK = "fsg2019"
DT = 0.05
B_SMALL = 3
# N = 1: one terminal step, one k-step of the SYRK.  N = 3: 3N = 9, ksteps = 3 < the unroll of 8, one partial tile.  N = 9: 2N = 18,
# the second tile has two columns, pair I = 1 starts at k-step 6 of 7.  N = 17: three tiles, 3N = 51.
N_SMALL = (1, 3, 9, 17)
N_MAX = {0: 97, 1: 96}      # the largest horizon the ABI takes (FSAEMPC_MAX_NV = 2N + ns)
TENSORS = dn.QP_KEYS
FACTOR, FLOOR, E64_MAX = 32.0, 1e-13, 1e-11


def exact_cases():
    """(model, N, integ, par): the four exact kernels ({kin, dyn} x {constants, parameter blocks}) under the three integrators at the
    small shapes; one instance at the largest horizon, default integrator, constants."""
    out = [(m, N, i, p) for m in (0, 1) for p in (False, True) for i in (0, 1, 2) for N in N_SMALL]
    return out + [(0, N_MAX[0], 1, False), (1, N_MAX[1], 2, False)]


def case_id(c):
    return "%s-N%d-integ%d-%s" % ("kin" if c[0] == 0 else "dyn", c[1], c[2], "par" if c[3] else "fixed")


def table():
    return dn.Table.load(os.path.join(ROOT, "fsae-mpc_amd", "tracks", TRACK + ".json"))


def inputs(model, N, integ, par):
    """x0 (B, nx), x_ref (B, N, nx), u (B, N, 2), P (B, 32) or None.  x0 and x_ref are fm.instances' (seed 31), u is uniform in
    [-2, 2] x [-0.08, 0.08], the blocks are param_draws(model, ids, 31, 0.1)."""
    import fsae_mpc_amd as fm
    B = 1 if N == N_MAX[model] else B_SMALL
    x0, _, _, xr = fm.instances(model, N, DT, table().L, 31, range(B))
    rng = np.random.default_rng(1000 * N + 100 * model + 10 * integ + int(par))
    u = np.stack([rng.uniform(-2, 2, (B, N)), rng.uniform(-0.08, 0.08, (B, N))], axis=2)
    return x0, xr, u, (fm.param_draws(model, np.arange(B), 31, 0.1) if par else None)


@functools.lru_cache(maxsize=None)
def reference(model, N, integ, par):
    """dict(inputs, ld: the long-double QP per instance, e64: {tensor: (B,) gaps of the float64 run}, with "Bd" for the diagonal
    blocks of Phi).  Callers leave it unchanged."""
    x0, xr, u, P = inputs(model, N, integ, par)
    tab = table()
    ld, e64 = [], {k: [] for k in TENSORS + ("Bd",)}
    for b in range(x0.shape[0]):
        Pb = None if P is None else P[b]
        ql = dn.exact_qp(tab, model, x0[b], u[b], xr[b], DT, integ, Pb, np.longdouble)
        q64 = dn.exact_qp(tab, model, x0[b], u[b], xr[b], DT, integ, Pb, np.float64)
        for k in e64:
            e64[k].append(dn.gap(q64[k], ql[k]))
        ld.append(ql)
    return dict(x0=x0, x_ref=xr, u=u, P=P, ld=ld, e64={k: np.array(v) for k, v in e64.items()})


def tolerance(e64):
    """Per tensor: 32 e64, at least 1e-13, e64 being the largest gap over the instances of the case's batch (the tensors are batch
    tensors; the rounding error of one instance is a single draw, and where a tensor cancels -- `const` sums (aff - x_ref)^2 with
    aff near 300 m and residuals near 0.1 m -- one draw can sit a hundred times below the next).  The factor covers what legitimately differs in the kernel: the summation
    order of the MFMA SYRK and of the row sweeps, FMA contraction and the device libm's 1-2 ulp sin / cos / atan / tan / pow / exp."""
    return np.maximum(FACTOR * np.asarray(e64), FLOOR)


# ---- reproducibility ----
REPRO_N, REPRO_B, REPRO_SEED = 20, 16, 31
REPRO_BLOCKS = [1] * 4 + [2] * 4 + [4] * 2


def repro_cases():
    """(kind, model, integ, par) over the twelve instantiations of the build kernel: {kin, dyn} x {plain, exact, blocked} x
    {constants, parameter blocks}, plain and exact under the three integrators, blocked under the model's default (-1)."""
    out = []
    for kind in ("plain", "exact", "blocked"):
        for m in (0, 1):
            for p in (False, True):
                out += [(kind, m, i, p) for i in ((-1,) if kind == "blocked" else (0, 1, 2))]
    return out


def repro_id(c):
    return "%s-%s-integ%d-%s" % (c[0], "kin" if c[1] == 0 else "dyn", c[2], "par" if c[3] else "fixed")


class ReproBuilds:
    """The builds of repro_cases() at N = 20, B = 16, seed 31 on the current device; run(case, fill) returns the raw 64-bit words of
    every output tensor.  fill: None (torch.empty), 0 or 0xFF: the byte the outputs are pre-filled with."""

    def __init__(self):
        import torch
        import fsae_mpc_amd as fm
        self.torch, self.fm = torch, fm
        self.tr = fm.Track.load(TRACK)
        self._inp, self._other = {}, None

    def _inputs(self, model):
        if model not in self._inp:
            up = lambda v: self.torch.from_numpy(np.ascontiguousarray(v)).cuda()
            x0, xl, ul, xr = (up(v) for v in self.fm.instances(model, REPRO_N, DT, self.tr.L, REPRO_SEED, range(REPRO_B)))
            self._inp[model] = (x0, xl, ul, xr, self.fm.param_draws(model, range(REPRO_B), REPRO_SEED, 0.1))
        return self._inp[model]

    def unrelated_step(self):
        """A fused dynamic N = 40 step: leaves other LDS and register contents behind."""
        fm, torch = self.fm, self.torch
        if self._other is None:
            up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
            x0, xl, ul, xr = (up(v) for v in fm.instances(fm.DYNAMIC, 40, DT, self.tr.L, 7, range(REPRO_B)))
            self._other = (fm.LtvBatch(fm.DYNAMIC, 40, DT, self.tr, REPRO_B), x0, xr, xl, ul)
        mpc, x0, xr, xl, ul = self._other
        mpc.step(x0, xr, xl, ul)
        torch.cuda.synchronize()

    def run(self, case, fill=None):
        kind, model, integ, par = case
        fm, torch = self.fm, self.torch
        x0, xl, ul, xr, P = self._inputs(model)
        kw = dict(integrator=integ, params=P if par else None)
        if kind == "exact":
            obj = fm.SqpBatch(model, REPRO_N, DT, self.tr, REPRO_B, **kw)
        else:
            obj = fm.LtvBatch(model, REPRO_N, DT, self.tr, REPRO_B, blocking=REPRO_BLOCKS if kind == "blocked" else None, **kw)
        if fill is not None:
            obj._f64 = lambda *shape: torch.full((int(np.prod(shape)) * 8,), fill, dtype=torch.uint8, device="cuda").view(torch.float64).view(*shape)
        q = obj.build_qp(x0, xr, ul) if kind == "exact" else obj.build_qp(x0, xr, xl, ul)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy().view(np.uint64) for k, v in q.items()}
