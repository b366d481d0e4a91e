"""numpy restatement of the three steps that put the batched SQP into the closed loop: the shift of the kept plan into the
start of a period's solve, the skip mask, and the take-over of the SQP's result.  Copies and selections only, so the device's results
are compared with these bit for bit.  Test infrastructure: it shares no code with the product."""
import numpy as np

STATUSES = (0, 1, 2, -1, -2, 4)     # converged, sweep limit, no step accepted, QP failed, QP infeasible, skipped


def shift(u_keep, shift=1):
    """u_keep (B, N, 2) -> u_init: stage k takes stage k + 1, the last stage is repeated; shift = 0 copies."""
    u = np.array(u_keep, dtype=np.float64)
    if shift:
        u[:, :-1] = u_keep[:, 1:]
    return u


def skip(finished, B):
    """(B,) int32: 1 where the car no longer drives (finished None: nobody is skipped)."""
    return np.zeros(B, dtype=np.int32) if finished is None else (np.asarray(finished) != 0).astype(np.int32)


def exitflag(status):
    """What the loop, the plant and the lap report read: 0 for status 0 and 1, the status itself otherwise."""
    status = np.asarray(status)
    return np.where((status == 0) | (status == 1), 0, status).astype(np.int32)


def accept(x_new, u_new, status, qp_iter, skip_, x_keep, u_keep):
    """(x_keep', u_keep', exitflag, iter).  x_new (B, Lx), u_new (B, Lu); qp_iter and skip_ may be None.  A skipped car keeps its
    plan and gets exit flag 0, iter 0; every other car takes the new plan over iff all of its entries are finite, whatever the status."""
    B = x_new.shape[0]
    sk = np.zeros(B, dtype=bool) if skip_ is None else np.asarray(skip_) != 0
    fin = np.isfinite(x_new.reshape(B, -1)).all(axis=1) & np.isfinite(u_new.reshape(B, -1)).all(axis=1)
    take = fin & ~sk
    xk, uk = np.array(x_keep, dtype=np.float64), np.array(u_keep, dtype=np.float64)
    xk[take] = x_new.reshape(xk.shape)[take]
    uk[take] = u_new.reshape(uk.shape)[take]
    ef = np.where(sk, 0, exitflag(status)).astype(np.int32)
    it = np.where(sk, 0, np.zeros(B, dtype=np.int32) if qp_iter is None else qp_iter).astype(np.int32)
    return xk, uk, ef, it
