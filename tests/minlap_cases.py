"""The fixtures of the minimum-time line's tests, shared by tests/test_minlap_cpu.py (which vets every one of them on the
CPU) and tests/test_minlap_gpu.py: lines for the lap-gradient kernel and starts for one iteration and the loop."""
import numpy as np

import minlap_numpy as mn
import plan_numpy as pn
import raceline_numpy as rn

W = 0.5            # the box of the fixtures, +-W: margin 0.25 off the default N_MAX 0.75
MARGIN = 0.25
_C = {}

# (track, model, N_s, N_c, v_cap, grip): the lines are the oracle's minimum-curvature lines in +-W
#   (37, 9)    N_s no multiple of 64 and fewer cells than lanes
#   (64, 16)   one full trip of the cell loops
#   (128, 32)  two trips
#   (130, 32)  a ragged last trip
#   v_cap = 9  capped cells
GRAD_CASES = [
    ("fss2019", 1, 128, 32, 20.0, 1.0),
    ("fso2020", 1, 37, 9, 20.0, 1.0),
    ("fsg2019", 0, 64, 16, 20.0, 1.0),
    ("fss2019", 0, 130, 32, 20.0, 0.8),
    ("fsg2019", 0, 128, 32, 9.0, 1.0),
    ("fsg2019", 1, 130, 32, 9.0, 0.8),
    ("fso2020", 1, 330, 128, 20.0, 1.0),
]
# The first minimum of the tracks' own lines lies nowhere near s = 0, so this one runs on a spike: every control point 0 but c_0 = 2 m at
# a knot spacing of 3 m, the tightest point of the line is then cell 0 (test_minlap_cpu.py asserts it) and both chains start at the wrap.
WRAP_CASE = ("fso2020", 1, 330, 128, 20.0, 1.0)
# starts of one iteration and of the loop, vetted to gain at least 0.05 s in one step with a clear winner
STEP_CASES = [
    ("fss2019", 1, 128, 32, 20.0, 1.0),
    ("fso2020", 1, 37, 9, 20.0, 1.0),
    ("fsg2019", 0, 128, 32, 9.0, 1.0),
]
# categories of branch decisions whose two sides must differ by more than 1e-9 relative in every fixture: the min of the two passes,
# |k| against 1e-12, sqrt(A_lat / K) against v_cap, and the branches of the longitudinal limit (polygon edges, U_ACC_MAX).  y against 1
# is not among them: a source cell that runs at its own corner speed has y = v^2 K / A_lat = 1 to the last bit BY CONSTRUCTION, and there
# both branches give the same total derivative (d y = 0 along vlat(K)); DESIGN.md 6o.
VETTED = ("pass", "k", "cap", "edge")


def kappa(orc, otr, N_s):
    key = ("k", otr.name, N_s)
    if key not in _C:
        k = pn.kappa_cells(orc, otr, N_s); k.setflags(write=False)
        _C[key] = k
    return _C[key]


def mincurv(orc, otr, N_s, N_c, w=W):
    """The oracle's minimum-curvature line in +-w, computed once and left unchanged."""
    key = ("c", otr.name, N_s, N_c, w)
    if key not in _C:
        H, g = rn.qp(orc, otr, N_s, N_c)
        x, f, flag, it, lam = orc.qp_solve(H, g, np.zeros((0, N_c)), np.full(N_c, -w), np.full(N_c, w), np.zeros(0), np.zeros(0))
        assert flag == 0
        x.setflags(write=False)
        _C[key] = x
    return _C[key]


def line(orc, otr, case):
    """The control points a case runs on."""
    name, model, N_s, N_c, v_cap, grip = case
    if case == WRAP_CASE:
        c = np.zeros(N_c); c[0] = 2.0
        return c
    return mincurv(orc, otr, N_s, N_c)


def restated(orc, otr, case, c=None, par=None):
    """minlap_numpy.lap_gradient of a case (on its own line, or on c), computed once per (case, line, block)."""
    name, model, N_s, N_c, v_cap, grip = case
    key = ("r", case, None if c is None else c.tobytes(), None if par is None else np.asarray(par).tobytes())
    if key not in _C:
        _C[key] = mn.lap_gradient(model, kappa(orc, otr, N_s), otr.L, line(orc, otr, case) if c is None else c, v_cap, grip, par, want_pairs=True)
    return _C[key]
