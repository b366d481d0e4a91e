"""Numpy statement of the planner stand-in of DESIGN.md 6i (fsaempc_plan_profile_batch_device), operation for operation: curvature
of the track table per cell (orc.kappa), the grip-limited corner speed, one forward and one backward pass under the longitudinal
limit the controller's own QP rows carry, then the 8 planner values and the traversal time of each cell.  The walk that resamples
a plan in time is the oracle's obtain_reference plus the state layout of the model (`reference`)."""
import numpy as np

from param_numpy import IDX

# the defaults of the entries the planner reads (include/fsaempc.h FSAEMPC_P_*; the same for both models)
DEFAULTS = dict(LF=0.8672, LR=0.6183, U_ACC_MAX=10.0, ALAT_MAX=5.0, ELL_LONG=10.0, ELL_LAT=9.163)
# first-quadrant vertices of the inscribed 12-gon of dynamic_tyre_linearise_constraints.m:18-23
POLY_C = (1.0, 0.8660254037844386, 0.5, 0.0)
POLY_S = (0.0, 0.5, 0.8660254037844386, 1.0)


def constants(par=None):
    """LF, LR and the limits from a parameter block (32,) or the defaults."""
    if par is None:
        return dict(DEFAULTS)
    return {k: float(par[IDX[k]]) for k in DEFAULTS}


def kappa_cells(orc, track, N_s):
    ds = track.L / N_s
    return np.array([orc.kappa(track, float(i) * ds) for i in range(N_s)])


def a_lat(model, c, grip):
    return grip * (c["ELL_LAT"] if model == 1 else c["ALAT_MAX"])


def a_x(model, c, grip, A_lat, v, K):
    """Largest longitudinal acceleration at speed v in a cell of curvature magnitude K."""
    if model == 0:
        return grip * c["U_ACC_MAX"]
    y = min(v * v * K / A_lat, 1.0)
    j = 0 if y <= POLY_S[1] else (1 if y <= POLY_S[2] else 2)
    X = POLY_C[j] + (POLY_C[j + 1] - POLY_C[j]) * (y - POLY_S[j]) / (POLY_S[j + 1] - POLY_S[j])
    return min(c["U_ACC_MAX"], grip * c["ELL_LONG"] * X)


def profile(model, k, L, v_cap=20.0, grip=1.0, par=None):
    """k: (N_s,) curvature of the cells at s_i = i ds.  Returns a dict: table (N_s, 8), t (N_s,), ds, v, vlat, K, i0."""
    k = np.asarray(k, dtype=np.float64)
    N_s = k.size
    ds = L / N_s
    c = constants(par)
    A_lat = a_lat(model, c, grip)
    K = np.maximum(np.abs(k), 1e-12)
    vlat = np.minimum(v_cap, np.sqrt(A_lat / K))
    i0 = int(np.argmin(vlat))                 # (the first index of the minimum)
    v = vlat.copy()
    for j in range(1, N_s + 1):
        i = (i0 + j) % N_s; p = (i0 + j - 1) % N_s
        v[i] = min(v[i], np.sqrt(v[p] * v[p] + 2.0 * a_x(model, c, grip, A_lat, v[p], K[p]) * ds))
    for j in range(1, N_s + 1):
        i = (i0 - j) % N_s; n = (i0 - j + 1) % N_s
        v[i] = min(v[i], np.sqrt(v[n] * v[n] + 2.0 * a_x(model, c, grip, A_lat, v[n], K[n]) * ds))
    vn = np.roll(v, -1)
    delta = np.arctan((c["LR"] + c["LF"]) * k)
    t = ds / v
    table = np.zeros((N_s, 8))
    table[:, 2] = v
    table[:, 4] = v * k
    table[:, 5] = delta
    table[:, 6] = (vn * vn - v * v) / (2.0 * ds)
    table[:, 7] = (np.roll(delta, -1) - delta) / t
    return dict(table=table, t=t, ds=ds, v=v, vlat=vlat, K=K, k=k, i0=i0, A_lat=A_lat, c=c)


def model_layout(model, r7):
    """obtain_reference's 7 x N rows in the state layout of the model: dynamic as they are, kinematic [s, n, mu, hypot(x_d, y_d), delta]."""
    r7 = np.asarray(r7)
    if model == 1:
        return r7
    return np.vstack([r7[0], r7[1], r7[2], np.hypot(r7[3], r7[4]), r7[6]])


def reference(orc, model, table, t, ds, s0, dt, N):
    """x_ref (nx, N) of a car at s0 on the plan (table (N_s, 8), t (N_s,)): the oracle's walk plus the layout."""
    N_s = np.asarray(t).size
    return model_layout(model, orc.obtain_reference(np.asarray(table).reshape(-1), ds, N_s, t, float(s0), dt, N))
