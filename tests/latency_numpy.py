"""Numpy / plain-Python statement of the imperfect closed loop, sharing no code with the product: Philox4x32-10, the
word -> normal map, the counter layout of the draws, the observation, the prediction through tests/param_numpy.psi and the slot schedule of
the plan history.  tests/test_latency_cpu.py pins the generator to the published known-answer vectors and csrc/cl_latency.h (on the host,
under the sanitizers) to this file; tests/test_latency_gpu.py pins the kernels to it."""
import math

import numpy as np

import param_numpy as pp

MAX_DELAY = 4
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
# (counter, key, output) of Philox4x32-10 as published with the generator (Random123's known-answer file)
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((MASK,) * 4, (MASK,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def philox(ctr, key):
    c0, c1, c2, c3 = [int(v) & MASK for v in ctr]
    k0, k1 = [int(v) & MASK for v in key]
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def words(seed, cid, step, j):
    return philox((step & MASK, j, cid & MASK, cid >> 32), (seed & MASK, seed >> 32))


def normals(w):
    z = []
    for h in range(2):
        u1, u2 = (w[2 * h] + 0.5) * 2.0 ** -32, (w[2 * h + 1] + 0.5) * 2.0 ** -32
        r, a = math.sqrt(-2.0 * math.log(u1)), 2 * math.pi * u2
        z += [r * math.cos(a), r * math.sin(a)]
    return z


def draws8(seed, cid, step):
    """All eight normals of (seed, id, step): components 0 .. 3 from call 0, 4 .. 7 from call 1 (the models use the first nx)."""
    return np.array(normals(words(seed, cid, step, 0)) + normals(words(seed, cid, step, 1)))


def noise(nx, B, seed, id0, step):
    return np.array([draws8(seed, id0 + b, step)[:nx] for b in range(B)])


def observe(x0, sigma, finished, seed, id0, step):
    """x0 (B, nx), sigma None, (nx,) or (B, nx), finished (B,) or None."""
    x0 = np.asarray(x0, dtype=np.float64)
    B, nx = x0.shape
    out = x0.copy()
    if sigma is None:
        return out
    sg = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (B, nx))
    z = noise(nx, B, seed, id0, step)
    for b in range(B):
        if finished is not None and finished[b] != 0:
            continue
        for i in range(nx):
            if sg[b, i] > 0 and np.isfinite(sg[b, i]):
                out[b, i] = x0[b, i] + sg[b, i] * z[b, i]
    return out


def slot(delay, step, lag):
    return (step - lag) % (delay + 1)


def resolve_integrator(model, integ):
    return integ if integ >= 0 else (pp.RK2 if model == 0 else pp.RK4)


def predict(P, orc, model, track, x_obs, u_hist, delay, step, dt, integ):
    """x_obs (nx,) of one car rolled over `delay` periods; u_hist (delay + 1, N, 2) of that car.  P: the controller's block (32,).
    Returns x_obs itself when an input or the result is not finite."""
    x = np.array(x_obs, dtype=np.float64)
    integ = resolve_integrator(model, integ)
    with np.errstate(all="ignore"):
        for j in range(delay):
            u = u_hist[slot(delay, step, delay - j), 0]
            if not np.isfinite(u).all():
                return np.array(x_obs, dtype=np.float64)
            x = pp.psi(P, orc, model, track, x, u, dt, integ)
            if not np.isfinite(x).all():
                return np.array(x_obs, dtype=np.float64)
    return x


def schedule(delay, periods):
    """The loop's bookkeeping on tagged plans: per period the tag the plant reads and the tags of the predictor's inputs."""
    hist = ["initial"] * (delay + 1)
    plant, pred = [], []
    for k in range(periods):
        pred.append([hist[slot(delay, k, delay - j)] for j in range(delay)])   # the observe step runs before the solve
        hist[slot(delay, k, 0)] = k                                            # the accepted plan goes to its slot
        plant.append(hist[slot(delay, k, delay)])
    return plant, pred
