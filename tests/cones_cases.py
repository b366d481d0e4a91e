"""Cases shared by tests/test_cones_cpu.py and tests/test_cones_gpu.py: the cone maps of the three tracks
(tests/golden/tracks/cones.npz), the restatement's tables for them (computed once and left unchanged), and the constructions of
the invariance and known-answer tests."""
import os

import numpy as np

import cones_numpy as cq

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TRACKS = ["fsg2019", "fss2019", "fso2020"]
MARGIN, REACH = 0.7, 5.0


def cone_maps():
    z = np.load(os.path.join(ROOT, "tests", "golden", "tracks", "cones.npz"))
    return {t: (z[t + "_left"], z[t + "_right"]) for t in TRACKS}


_CACHE = {}


def reference_case(name, N_w):
    """(track, left, right, n_lo, n_hi, info) of the restatement at margin 0.7, computed once per (track, N_w) and left unchanged"""
    import fsae_mpc_amd as fm
    if (name, N_w) not in _CACHE:
        tr = fm.Track.load(name)
        left, right = cone_maps()[name]
        lo, hi, inf = cq.corridor_from_cones(tr, tr.L, left, right, N_w, MARGIN, REACH)
        for a in (lo, hi, inf):
            a.setflags(write=False)
        _CACHE[(name, N_w)] = (tr, left, right, lo, hi, inf)
    return _CACHE[(name, N_w)]


def insert_on_chords(c, m=2):
    """m points on every chord of the closed polyline through c, evenly spaced: ((m + 1) K, 2)"""
    nxt = np.roll(c, -1, axis=0)
    return np.stack([c + (nxt - c) * (k / (m + 1.0)) for k in range(m + 1)], axis=1).reshape(-1, 2)


def known_answer_cones(tr, N_w, K, sign):
    """K cones at p(s_k) + w_k N(s_k), s_k on a subset of the cell positions, w_k = sign (1 + 0.5 sin(10 pi s_k / L)): (cells, cones, w)"""
    cells = np.unique(np.floor(np.arange(K) * N_w / K).astype(np.int64))
    s = cells * (tr.L / N_w)
    w = sign * (1 + 0.5 * np.sin(10 * np.pi * s / tr.L))
    p, _, N = cq.frame(tr, s)
    return cells, p + w[:, None] * N, w
