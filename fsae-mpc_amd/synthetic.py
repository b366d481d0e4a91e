"""Synthetic LTV-MPC instances of SURVEY 8(d): splitmix64 keyed by seed ^ (id * 0x9E3779B97F4A7C15),
u01 = (next() >> 11) * 2^-53.  Product-side generator (numpy, vectorised over the batch); the oracle has an
independent C copy and tests/ check the two agree bit for bit."""
import numpy as np

KINEMATIC, DYNAMIC = 0, 1
_GOLD = np.uint64(0x9E3779B97F4A7C15)


def _next(state):
    with np.errstate(over="ignore"):
        state += _GOLD
        z = state.copy()
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _u01(state):
    return (_next(state) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def reference_live(x0, N, dt, target_vel=20.0):
    """main.m:107-114: velocity ramp +-10 m/s^2 clipped at TARGET_VEL, s_ref = s0 + cumsum(v_ref*dt).
    x0: (B, nx) -> x_ref (B, N, nx) (per-instance memory = nx x N column-major)."""
    B, nx = x0.shape
    k = np.arange(1, N + 1, dtype=np.float64)[None, :]
    v0 = x0[:, 3:4]
    up = np.minimum(v0 + 10 * dt * k, target_vel)
    dn = np.maximum(v0 - 10 * dt * k, target_vel)
    v = np.where(v0 < target_vel, up, dn)
    x_ref = np.zeros((B, N, nx))
    x_ref[:, :, 3] = v
    x_ref[:, :, 0] = x0[:, 0:1] + np.cumsum(v * dt, axis=1)
    return x_ref


def instances(model, N, dt, L, seed, ids):
    """Returns x0 (B,nx), x_lin (B,N,nx), u_lin (B,N,2), x_ref (B,N,nx); per-instance memory is the
    column-major nx x N / 2 x N array the C ABI expects."""
    ids = np.asarray(ids, dtype=np.uint64)
    nx = 5 if model == KINEMATIC else 7
    with np.errstate(over="ignore"):
        st = np.uint64(seed) ^ (ids * _GOLD)
    s0 = _u01(st) * L
    n0 = -0.5 + _u01(st)
    mu0 = -0.1 + 0.2 * _u01(st)
    v0 = 5 + 15 * _u01(st)
    d0 = -0.1 + 0.2 * _u01(st)
    B = len(ids)
    x0 = np.zeros((B, nx))
    if model == KINEMATIC:
        x0[:, 0], x0[:, 1], x0[:, 2], x0[:, 3], x0[:, 4] = s0, n0, mu0, v0, d0
    else:
        yd = -0.2 + 0.4 * _u01(st)
        td = -0.3 + 0.6 * _u01(st)
        x0[:, 0], x0[:, 1], x0[:, 2], x0[:, 3], x0[:, 4], x0[:, 5], x0[:, 6] = s0, n0, mu0, v0, yd, td, d0
    x_lin = np.repeat(x0[:, None, :], N, axis=1).copy()
    x_lin[:, :, 0] = s0[:, None] + v0[:, None] * dt * np.arange(N)[None, :]
    u_lin = np.zeros((B, N, 2))
    x_ref = reference_live(x0, N, dt, 20.0)
    return x0, x_lin, u_lin, x_ref


_PAR_SALT = np.uint64(0xD1B54A32D192ED03)
_PAR_REL = list(range(0, 4)) + list(range(5, 8)) + list(range(9, 15)) + list(range(19, 28))   # drawn within +-spread of the default
_PAR_LOG = list(range(15, 19))                                                               # slack costs: scaled by 10^U(-1, 1)


def param_draws(model, ids, seed, spread):
    """One parameter block per instance id (fsaempc_ltv_params, PARAM_INDEX): a pure function of (model, id, seed, spread), so the
    shards of a multi-GPU run draw the same cars as the single-GPU run.  Entries 0-3 (M, IZ, LF, LR), 5-7 (PB, PC, PD), 9-14 (cost
    weights) and 19-27 (limits, ellipse axes) are uniform within +-spread (relative) of the default, the slack costs 15-18 are
    scaled by 10^U(-1, 1); GRAV, PE and the plant's PID entries stay at their defaults.  splitmix64 keyed by the id, as for
    instances(), with a salt of its own.  Returns (len(ids), 32)."""
    from ._lib import NPAR, default_params
    ids = np.asarray(ids, dtype=np.uint64)
    with np.errstate(over="ignore"):
        st = (np.uint64(seed) ^ (ids * _GOLD)) ^ _PAR_SALT
    out = np.repeat(default_params(model)[None, :], len(ids), axis=0)
    assert out.shape[1] == NPAR
    for j in _PAR_REL:
        out[:, j] *= 1.0 + spread * (2.0 * _u01(st) - 1.0)
    for j in _PAR_LOG:
        out[:, j] *= 10.0 ** (2.0 * _u01(st) - 1.0)
    return out


_CONE_SALT = np.uint64(0x8CB92BA72F3D8DD7)


def cone_draws(left, right, sigma, P, seed):
    """P noisy copies of a cone map for a Monte-Carlo over perception noise (Corridor.from_cones takes them as they are): left (K_l, 2)
    and right (K_r, 2) -> (P, K_l, 2), (P, K_r, 2) with independent Gaussian noise of standard deviation sigma on every coordinate.  A
    pure function of (the maps, sigma, P, seed): splitmix64 keyed by the copy, as for instances(), with a salt of its own, and
    Box-Muller on pairs of its uniforms.  sigma = 0 gives P copies."""
    left, right = np.asarray(left, dtype=np.float64).reshape(-1, 2), np.asarray(right, dtype=np.float64).reshape(-1, 2)
    if int(P) != P or P < 1:
        raise ValueError("P must be an integer >= 1, got %r" % (P,))
    if not (np.isfinite(sigma) and sigma >= 0):
        raise ValueError("sigma must be finite and >= 0, got %r" % (sigma,))
    P = int(P)
    with np.errstate(over="ignore"):
        st = (np.uint64(seed) ^ (np.arange(P, dtype=np.uint64) * _GOLD)) ^ _CONE_SALT
    out = []
    for m in (left, right):
        z = np.zeros((P,) + m.shape)
        for k in range(m.shape[0]):
            u1, u2 = _u01(st), _u01(st)
            r = np.sqrt(-2.0 * np.log(1.0 - u1))           # (u1 in [0, 1): the logarithm's argument is in (0, 1])
            z[:, k, 0], z[:, k, 1] = r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)
        out.append(m[None, :, :] + sigma * z if sigma > 0 else np.repeat(m[None, :, :], P, axis=0))
    return out[0], out[1]
