"""numpy restatement of the lap gate, written from the rules of include/fsaempc.h (FSAEMPC_LS_*), and the cars, tracks
and oracle drive of the multi-lap tests.  Test infrastructure: it shares no code with the product.

gate() works in place on one period's arrays: x0 (B, nx), x_ref (B, N, nx), x_keep (B, N, nx), finished (B,) int, lap_state (B, 4),
lap_times (B, laps), and optionally metrics (B, 16) with lap_records (B, laps, 16)."""
import numpy as np

import lap_numpy as ln

DONE, STEPS, S_PREV, T_CROSS = 0, 1, 2, 3
STATE = ["DONE", "STEPS", "S_PREV", "T_CROSS"]


def gate(dt, L, laps, x0, x_ref, x_keep, finished, lap_state, lap_times, metrics=None, lap_records=None):
    assert (metrics is None) == (lap_records is None)
    for b in range(x0.shape[0]):
        ls = lap_state[b]
        fin = int(finished[b])
        if fin == 2 or (fin == 1 and ls[DONE] >= laps):
            continue
        if fin == 1:
            k, s = ls[STEPS], x0[b, 0]
            f = 1.0
            if k > 0 and s > ls[S_PREV]:
                f = min(max((L - ls[S_PREV]) / (s - ls[S_PREV]), 0.0), 1.0)
            t = (k - 1 + f) * dt if k > 0 else 0.0
            lap_times[b, int(ls[DONE])] = t - ls[T_CROSS]
            ls[T_CROSS] = t
            ls[DONE] += 1
            if ls[DONE] < laps:
                if metrics is not None:
                    lap_records[b, int(ls[DONE]) - 1] = metrics[b]
                    lap_records[b, int(ls[DONE]) - 1, ln.IDX["STATUS"]] = 1.0
                    metrics[b] = 0.0
                x0[b, 0] = x0[b, 0] - L
                x_ref[b, :, 0] = x_ref[b, :, 0] - L
                x_keep[b, :, 0] = x_keep[b, :, 0] - L
                finished[b] = 0
        if finished[b] == 0:
            ls[S_PREV] = x0[b, 0]
            ls[STEPS] += 1


def fresh(B, laps, metrics=False):
    """(lap_state, lap_times, lap_records) as the caller of the gate prepares them"""
    return np.zeros((B, 4)), np.full((B, laps), np.nan), (np.zeros((B, laps, 16)) if metrics else None)


def summary(lap_times):
    """(laps, 4): cars that completed the lap, mean, min, max of its time over them"""
    lap_times = np.asarray(lap_times, dtype=np.float64)
    out = np.full((lap_times.shape[1], 4), np.nan)
    for l in range(lap_times.shape[1]):
        v = lap_times[:, l][~np.isnan(lap_times[:, l])]
        out[l, 0] = v.size
        if v.size:
            out[l, 1:] = [np.sum(v) / v.size, v.min(), v.max()]
    return out


# ---- test A: the gate alone on hand-made arrays ---------------------------------------------------------------------------------
GATE_L, GATE_DT, GATE_LAPS, GATE_CALLS, GATE_NX, GATE_N = 100.0, 0.05, 3, 6, 5, 3
GATE_KINDS = ["crosses at calls 2 and 4", "crosses thrice, final", "never crosses", "lost from the start", "crosses at the first call"]


def gate_script(B):
    """What a pre-step would leave on each of the six calls for B cars of the five kinds (index b % 5; calls count from 0): s (calls, B) and
    finished (calls, B) as the pre-step sets it GIVEN the gate's resets (a pre-step only ever raises the flag), so the driver below ORs it
    into the carried flag.  Each group of five gets its own small offset in s, so neighbouring lanes of a kind hold different numbers; the
    offsets repeat after twelve groups, so car 60 + i is car i again."""
    kind = np.arange(B) % 5
    off = 0.001 * ((np.arange(B) // 5) % 12)
    s_of = {   # s as seen by the pre-step: the car's arc length in the lap it is driving
        0: [90.0, 95.0, 100.5, 4.0, 101.25, 3.0],
        1: [97.0, 100.25, 100.75, 100.125, 0.0, 0.0],      # crosses at calls 1, 2 and 3 (the third is final); held afterwards
        2: [10.0, 11.0, 12.0, 13.0, 14.0, 15.0],
        3: [0.0, 0.0, 0.0, 0.0, 0.0, 0.0],                  # the pre-step's placeholder
        4: [100.5, 1.5, 2.5, 3.5, 4.5, 5.5],
    }
    s = np.stack([np.array(s_of[k]) for k in kind], axis=1) + off[None, :] * (kind != 3)[None, :]
    raise_ = s >= GATE_L
    lost = np.broadcast_to(kind == 3, s.shape)
    return kind, s, raise_, lost


def gate_inputs(B, call, s, raise_, lost, finished):
    """The arrays before call `call`: x0, x_ref, x_keep built from s with distinct values everywhere, finished = carried flag raised"""
    rng = np.random.default_rng(100 + call)
    x0 = rng.uniform(-1, 1, (B, GATE_NX)); x0[:, 0] = s[call]
    x_ref = rng.uniform(-1, 1, (B, GATE_N, GATE_NX)); x_ref[:, :, 0] = s[call][:, None] + 0.5 * np.arange(1, GATE_N + 1)[None, :]
    x_keep = rng.uniform(-1, 1, (B, GATE_N, GATE_NX)); x_keep[:, :, 0] = s[call][:, None] + 0.45 * np.arange(1, GATE_N + 1)[None, :]
    fin = finished.copy()
    fin[raise_[call] & (fin == 0)] = 1
    fin[lost[call]] = 2
    return x0, x_ref, x_keep, fin


# ---- test E: a short closed track ------------------------------------------------------------------------------------------------
CIRCLE = dict(radius=15.0, target_vel=8.0, points=64, M=40, B=8, N=10, laps=3, cap=300)


def circle_points():
    a = np.linspace(0.0, 2 * np.pi, CIRCLE["points"], endpoint=False)
    return CIRCLE["radius"] * np.cos(a), CIRCLE["radius"] * np.sin(a)


def circle_starts(L):
    """(s0, n0, v0) of the eight cars: 2 .. 9 m before the line (a lap is about 236 steps at the target speed, so the first crossing
    comes within 30 steps and the second, after a flying lap, within the cap), small lateral offsets, near the target speed"""
    return [(L - 2.0 - i, 0.1 * ((i % 3) - 1), 7.0 + 0.25 * i) for i in range(CIRCLE["B"])]


# ---- the oracle's closed loop with the gate in it --------------------------------------------------------------------------------
def drive_oracle_laps(orc, otr, model, N, dt, cart0, s0, v0, steps, laps, target_vel=20.0):
    """lap_numpy.drive_oracle with the gate between the pre-step and the step, one car at a time.  Returns the history (as there, plus
    `crossed` (T, B): the gate wrapped the car on this step), lap_state and lap_times."""
    nx, ns = orc.dims(model, N)[:2]
    B = cart0.shape[0]
    h = dict(x0=np.zeros((steps, B, nx)), finished=np.zeros((steps, B), dtype=int), flag=np.zeros((steps, B), dtype=int),
             iter=np.zeros((steps, B), dtype=int), fval=np.zeros((steps, B)), slack=np.zeros((steps, B, ns)), a=np.zeros((steps, B)),
             cart=np.zeros((steps, B, 7)), crossed=np.zeros((steps, B), dtype=bool))
    lap_state, lap_times, _ = fresh(B, laps)
    k = np.arange(1, N + 1) * dt
    for b in range(B):
        cart, pid = cart0[b].copy(), np.zeros(4)
        fin = np.zeros(1, dtype=int)
        x_opt = np.zeros((1, N, nx)); u_opt = np.zeros((N, 2))
        x_opt[0, :, 0] = 10 * k ** 2 / 2 + s0[b]; x_opt[0, :, 3] = 10 * k + v0[b]; u_opt[:, 0] = 10
        for t in range(steps):
            if fin[0] == 0:
                x0, x_ref, past = orc.cl_pre(model, N, dt, otr, cart, x_opt[0, 0, 0], target_vel)
                fin[0] = 2 if ln.is_lost(x0, cart) else (1 if past else 0)
                x0 = x0.reshape(1, nx); xr = np.ascontiguousarray(x_ref.T).reshape(1, N, nx)
                done = lap_state[b, DONE]
                gate(dt, otr.L, laps, x0, xr, x_opt, fin, lap_state[b:b + 1], lap_times[b:b + 1])
                h["crossed"][t, b] = lap_state[b, DONE] > done and fin[0] == 0
                h["x0"][t, b] = x0[0]
            h["finished"][t, b] = fin[0]
            h["cart"][t, b] = cart
            if fin[0]:
                continue
            u_new, x_new, slack, fval, flag, it = orc.ltv_step(model, otr, N, dt, x0[0], xr[0].T, x_opt[0].T, u_opt.T)
            if flag in (0, 1) and np.isfinite(x_new).all() and np.isfinite(u_new).all():
                x_opt, u_opt = x_new.reshape(1, N, nx).copy(), u_new.reshape(N, 2).copy()
            if np.isfinite(x_opt[0, 0, 3]) and np.isfinite(x_opt[0, 0, nx - 1]):
                cart, pid, _ = orc.plant_step(cart, pid, x_opt[0, 0, 3], x_opt[0, 0, nx - 1], dt)
            h["flag"][t, b], h["iter"][t, b], h["fval"][t, b], h["slack"][t, b], h["a"][t, b], h["cart"][t, b] = flag, it, fval, slack, u_opt[0, 0], cart
    return h, lap_state, lap_times
