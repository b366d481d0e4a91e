"""Move blocking (held inputs) restated in numpy, independent of the library and of the oracle: the blocking matrix E and the
blocked QP it implies.  With block lengths len_1 .. len_M (sum N) the input of step k is u_k = v_block(k); the QP's variables are
[v_1 .. v_M; slacks], so z = E z_b with E (2N + ns) x (2M + ns): a 2 x 2 identity from block(k) to step k, the identity on the slacks.

Batch layout = the device layout of the C ABI (tests/kkt_numpy.py): H (B, nV, nV), A (B, nV, nC) and Bt (B, nV, nx N) are the
memory of per-instance column-major matrices, i.e. indexed [b, column, row]."""
import numpy as np


def block_of_step(lens):
    return np.repeat(np.arange(len(lens)), lens)


def blocking_matrix(lens, ns):
    """E, (2N + ns) x (2M + ns)."""
    lens = [int(v) for v in lens]
    N, M = sum(lens), len(lens)
    E = np.zeros((2 * N + ns, 2 * M + ns))
    for k, j in enumerate(block_of_step(lens)):
        E[2 * k, 2 * j] = 1.0
        E[2 * k + 1, 2 * j + 1] = 1.0
    for s in range(ns):
        E[2 * N + s, 2 * M + s] = 1.0
    return E


def block_qp(q, E):
    """The blocked QP of the batch `q` (keys H, g, A, lb, ub, lbA, ubA; Bt, const, pred and whatever else is there pass through or
    are condensed alike): H_b = E'HE, g_b = E'g, A_b = AE, Bt_b = Bt E, the variable bounds of each column's first member, the rows'
    bounds unchanged."""
    first = np.array([np.nonzero(E[:, j])[0][0] for j in range(E.shape[1])])
    out = dict(q)
    out["H"] = np.einsum("ip,bji,jq->bqp", E, q["H"], E)          # [b, col q, row p] = sum_ij E[i,p] H[row i, col j] E[j,q]
    out["g"] = q["g"] @ E
    out["A"] = np.einsum("jq,bjr->bqr", E, q["A"])                # [b, col q, row r] = sum_j A[row r, col j] E[j,q]
    out["lb"] = q["lb"][:, first]
    out["ub"] = q["ub"][:, first]
    if "Bt" in q:
        out["Bt"] = np.einsum("jq,bjr->bqr", E, q["Bt"])
    return out
