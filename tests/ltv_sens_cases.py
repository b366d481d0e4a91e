"""The inputs shared by tests/test_ltv_sens_cpu.py and tests/test_ltv_sens_rows_gpu.py: deterministic batches of (x0, x_ref, x_lin,
u_lin) on which the solve of the LTV-MPC step has an active row in every family of the constraint block, the cotangent sets of the
step VJP, and the row families themselves.  Arrays are numpy in the oracle's layout, which is the device layout too: instance-major,
x_ref / x_lin (B, N, nx) and u_lin (B, N, 2), i.e. per instance the memory of the column-major nx x N / 2 x N array.

On fm.instances (seed 20190) alone no row of the delta block and hardly one of the v block is ever active, so the unit coefficients
of those rows in the VJP's chain would only be multiplied by zero.  The N = 8 batches therefore replace two thirds of the synthetic
instances: a slow car whose reference position lies far behind it (the cost weights states 0..2 only, so this is what makes the
plan brake into v >= V_MIN), and a steering angle next to its limit with a reference far to that side."""
import numpy as np

DT = 0.05
SEED = 20190
TRACK = "fsg2019"
B_ROWS, B_ODD, B_INFEASIBLE = 48, 32, 4
N_ROWS = 8                       # the smallest horizon at which the QP suite runs both models
CASES = [(0, 8), (1, 8), (0, 13), (1, 9)]     # (model, N): crafted thirds at N = 8; odd horizons off the tile sizes, synthetic
INFEASIBLE = (1, 2)              # the instances of infeasible_inputs() whose QP has no feasible point
COTANGENT_SETS = ("ubar", "xbar", "sbar", "fbar", "all", "all_k3")
FBAR_SCALE = 1e-3                # fval reaches 1e6 where the reference lies 200 m behind: keeps its share of a column comparable


def case_id(c):
    return "%s-N%d" % ("kin" if c[0] == 0 else "dyn", c[1])


def dims(model, N):
    """nx, ns, nV, nC of fsaempc_ltv_nx / _nV / _nC."""
    return (5, 1, 2 * N + 1, 6 * N) if model == 0 else (7, 4, 2 * N + 4, 20 * N)


def batch_size(model, N):
    return B_ROWS if N == N_ROWS else B_ODD


def _synthetic(model, N, B):
    import fsae_mpc_amd as fm
    tr = fm.Track.load(TRACK)
    x0, xl, ul, xr = fm.instances(model, N, DT, tr.L, SEED, range(B))
    return dict(x0=x0.copy(), x_ref=xr.copy(), x_lin=xl.copy(), u_lin=ul.copy())


def inputs(model, N):
    """dict(x0 (B, nx), x_ref (B, N, nx), x_lin (B, N, nx), u_lin (B, N, 2)) of the case.  At N = 8 the first third is the slow
    car, the second third the steering at its limit (alternating sides), the rest synthetic."""
    B = batch_size(model, N)
    d = _synthetic(model, N, B)
    if N != N_ROWS:
        return d
    nx = dims(model, N)[0]
    x0, xr, xl = d["x0"], d["x_ref"], d["x_lin"]
    third = B // 3
    for b in range(third):
        v = 0.3 + 0.05 * b
        x0[b, 3] = v
        xl[b, :, 3] = v
        xl[b, :, 0] = x0[b, 0] + v * DT * np.arange(N)
        xr[b, :, 0] = x0[b, 0] - 200.0
    for b in range(third, 2 * third):
        sgn = 1.0 if b % 2 else -1.0
        x0[b, nx - 1] = sgn * (0.38 - 0.002 * b)
        xl[b, :, nx - 1] = x0[b, nx - 1]
        xr[b, :, 1] = sgn * 3.0
        xr[b, :, 2] = sgn * 2.0
    return d


def infeasible_inputs(model):
    """Four synthetic instances at N = 8; instance 1 starts with its steering angle beyond DELTA_MAX, instance 2 with a negative
    speed (both repeated in x_lin): their QPs have no feasible point.  Instances 0 and 3 are untouched neighbours."""
    d = _synthetic(model, N_ROWS, B_INFEASIBLE)
    nx = dims(model, N_ROWS)[0]
    d["x0"][1, nx - 1] = 0.6
    d["x_lin"][1, :, nx - 1] = 0.6
    d["x0"][2, 3] = -1.0
    d["x_lin"][2, :, 3] = -1.0
    return d


def cotangents(model, N, B, name):
    """The cotangent set `name` for B instances: dict(ubar (B, k, 2N), xbar (B, k, nx N), sbar (B, k, ns), fbar (B, k)), None for a
    cotangent that is not given.  One of the four alone (k = 1), all four (k = 1), or all four with k = 3 independent columns."""
    nx, ns, _, _ = dims(model, N)
    k = 3 if name == "all_k3" else 1
    rng = np.random.default_rng([11, model, N, COTANGENT_SETS.index(name)])
    full = dict(ubar=rng.standard_normal((B, k, 2 * N)), xbar=rng.standard_normal((B, k, nx * N)), sbar=rng.standard_normal((B, k, ns)),
                fbar=rng.standard_normal((B, k)) * FBAR_SCALE)
    return {key: (v if name in ("all", "all_k3", key) else None) for key, v in full.items()}


def families(model, N):
    """Row family -> row indices of the constraint block, the layout that row_step / row_coef of csrc/ltv_build.hip decode: four
    blocks of N unit rows (v, delta, n twice), then kinematic: two blocks of N tyre rows; dynamic: two blocks of 2N slip rows (two
    rows per step) and 12 ellipse rows per step."""
    blk = lambda i, w=N: np.arange(i, i + w)
    f = dict(v=blk(0), delta=blk(N), n_a=blk(2 * N), n_b=blk(3 * N))
    if model == 0:
        f.update(tyre_a=blk(4 * N), tyre_b=blk(5 * N))
    else:
        f.update(slip_a=blk(4 * N, 2 * N), slip_b=blk(6 * N, 2 * N), ellipse=blk(8 * N, 12 * N))
    return f


def directions(model, N, B, x0, x_ref):
    """Random directions of x0 (B, nx) and x_ref (B, nx N) for the directional differences, scaled by the size of each entry."""
    rng = np.random.default_rng([13, model, N])
    v0 = rng.standard_normal(x0.shape) * np.maximum(1.0, np.abs(x0))
    xr = x_ref.reshape(B, -1)
    return v0, rng.standard_normal(xr.shape) * np.maximum(1.0, np.abs(xr))
