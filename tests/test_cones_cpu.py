"""CPU tests of the corridors from cone positions: the numpy restatement (tests/cones_numpy.py) against an independent
brute-force ray cast, its invariances and a known answer; the CSV reader of the cone columns; what the C entry refuses before any
launch; the noisy cone maps of the Monte-Carlo.  The cones are the rX, rY, lX, lY columns of the reference's three race-line CSVs,
kept in tests/golden/tracks/cones.npz."""
import ctypes as C
import os

import numpy as np
import pytest

import cones_numpy as cq
from cones_cases import MARGIN, REACH, TRACKS, cone_maps, insert_on_chords, known_answer_cones, reference_case

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


# ---- 1. the restatement against the ray cast -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("N_w", [64, 500])
@pytest.mark.parametrize("name", TRACKS)
def test_restatement_against_the_ray_cast(name, N_w):
    tr, left, right, lo, hi, inf = reference_case(name, N_w)
    el, hl = cq.ray_cast(tr, tr.L, left, N_w, +1, REACH)
    er, hr = cq.ray_cast(tr, tr.L, right, N_w, -1, REACH)
    assert (hl == 1).all() and (hr == 1).all(), (hl.min(), hl.max(), hr.min(), hr.max())
    dl, dr = np.abs(hi + MARGIN - el).max(), np.abs(lo - MARGIN - er).max()
    print(name, N_w, "restatement vs ray cast:", dl, dr, "least width", inf[7])
    assert dl <= 1e-12 and dr <= 1e-12
    assert (lo < 0).all() and (hi > 0).all() and inf[7] > 0
    assert inf[0] == len(left) and inf[1] == len(right)
    assert (inf[2:7] == 0).all(), inf
    assert inf[7] == (hi - lo).min()


# ---- 2. invariances ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TRACKS)
def test_a_permutation_of_the_cones_changes_no_bit(name):
    tr, left, right, lo, hi, inf = reference_case(name, 64)
    pl, pr = np.random.default_rng(11).permutation(len(left)), np.random.default_rng(12).permutation(len(right))
    lo2, hi2, inf2 = cq.corridor_from_cones(tr, tr.L, left[pl], right[pr], 64, MARGIN, REACH)
    assert lo2.tobytes() == lo.tobytes() and hi2.tobytes() == hi.tobytes() and inf2.tobytes() == inf.tobytes()


@pytest.mark.parametrize("name", TRACKS)
def test_points_inserted_on_every_chord_leave_the_tables(name):
    tr, left, right, lo, hi, inf = reference_case(name, 64)
    lo2, hi2, inf2 = cq.corridor_from_cones(tr, tr.L, insert_on_chords(left), insert_on_chords(right), 64, MARGIN, REACH)
    assert inf2[0] == 3 * len(left) and inf2[1] == 3 * len(right) and (inf2[2:7] == 0).all(), inf2
    assert np.abs(lo2 - lo).max() <= 1e-12 and np.abs(hi2 - hi).max() <= 1e-12, (np.abs(lo2 - lo).max(), np.abs(hi2 - hi).max())


# ---- 3. known answer -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 97, 300])
@pytest.mark.parametrize("name", TRACKS)
def test_known_answer(name, K):
    import fsae_mpc_amd as fm
    tr = fm.Track.load(name)
    N_w = 600
    cells, cl, wl = known_answer_cones(tr, N_w, K, +1)
    _, cr, wr = known_answer_cones(tr, N_w, K, -1)
    st, s, n = cq.project(tr, tr.L, cl, REACH)
    assert (st == cq.KEPT).all()
    s_want = cells * (tr.L / N_w)
    ds = np.abs((s - s_want + tr.L / 2) % tr.L - tr.L / 2).max()
    print(name, K, "s recovered to", ds, "n to", np.abs(n - wl).max())
    assert ds <= 1e-9 and np.abs(n - wl).max() <= 1e-9
    lo, hi, inf = cq.corridor_from_cones(tr, tr.L, cl, cr, N_w, MARGIN, REACH)
    assert inf[0] == len(cells) and inf[1] == len(cells) and (inf[2:5] == 0).all(), inf
    assert np.abs(hi[cells] - (wl - MARGIN)).max() <= 1e-9 and np.abs(lo[cells] - (wr + MARGIN)).max() <= 1e-9
    if K == 1:
        assert (hi == hi[0]).all() and (lo == lo[0]).all()


# ---- 4. the CSV reader ---------------------------------------------------------------------------------------------------------------
def write_csv(path, left, right, blank_left=()):
    with open(path, "w") as f:
        f.write("X,Y,vX,vY,aX,aY,dt,rX,rY,lX,lY\n")
        for k in range(len(left)):
            lpair = "," if k in blank_left else "%.17g,%.17g" % tuple(left[k])
            f.write("%d,0,0,0,0,0,0.1,%.17g,%.17g,%s\n" % ((k,) + tuple(right[k]) + (lpair,)))


@pytest.mark.parametrize("name", TRACKS)
def test_cones_from_csv_returns_the_same_doubles(tmp_path, name):
    import fsae_mpc_amd as fm
    left, right = cone_maps()[name]
    write_csv(tmp_path / "c.csv", left, right)
    l, r = fm.Track.cones_from_csv(str(tmp_path / "c.csv"))
    assert l.shape == left.shape and r.shape == right.shape
    assert l.tobytes() == np.ascontiguousarray(left).tobytes() and r.tobytes() == np.ascontiguousarray(right).tobytes()


def test_cones_from_csv_skips_an_empty_pair_on_its_side_only(tmp_path):
    import fsae_mpc_amd as fm
    left, right = cone_maps()["fsg2019"]
    write_csv(tmp_path / "c.csv", left, right, blank_left=(0, 5, len(left) - 1))
    l, r = fm.Track.cones_from_csv(str(tmp_path / "c.csv"))
    keep = np.setdiff1d(np.arange(len(left)), [0, 5, len(left) - 1])
    assert np.array_equal(l, left[keep]) and np.array_equal(r, right)
    (tmp_path / "n.csv").write_text("X,Y,vX,vY,aX,aY,dt,rX,rY,lX,lY\n0,0,0,0,0,0,0,nan,1,2,3\n1,0,0,0,0,0,0,4,5,6,inf\n2,0,0,0,0,0,0,7,8,9,10\n")
    l, r = fm.Track.cones_from_csv(str(tmp_path / "n.csv"))
    assert np.array_equal(l, [[2, 3], [9, 10]]) and np.array_equal(r, [[4, 5], [7, 8]])
    (tmp_path / "e.csv").write_text("X,Y,vX,vY,aX,aY,dt,rX,rY,lX,lY\n0,0,0,0,0,0,0,,,,\n")
    l, r = fm.Track.cones_from_csv(str(tmp_path / "e.csv"))
    assert l.shape == (0, 2) and r.shape == (0, 2)


def test_cones_from_csv_rejects_bad_input(tmp_path):
    import fsae_mpc_amd as fm
    with pytest.raises(fm.FsaempcError, match="cannot open"):
        fm.Track.cones_from_csv(str(tmp_path / "missing.csv"))
    p = tmp_path / "ten.csv"
    p.write_text("X,Y,vX,vY,aX,aY,dt,rX,rY,lX\n1,2,3,4,5,6,7,8,9,10\n")
    with pytest.raises(fm.FsaempcError, match="fewer than 11 columns"):
        fm.Track.cones_from_csv(str(p))
    L = fm.lib()
    n = C.c_int(0)
    pp = C.POINTER(C.c_double)()
    assert L.fsaempc_track_cones_from_csv(None, C.byref(pp), C.byref(n), C.byref(pp), C.byref(n)) == -1
    assert "null argument" in L.fsaempc_track_last_error().decode()
    L.fsaempc_track_cones_free(None)      # (free of nothing is allowed)


# ---- 5. the C entry's refusals -------------------------------------------------------------------------------------------------------
def test_the_entry_refuses_bad_arguments_before_a_launch():
    """Code and text of every refusal, in the entry's order.  The pointers are never read on the host, so small host buffers stand in
    for device memory; valid arguments get as far as the launch, which has no device here."""
    import fsae_mpc_amd as fm
    L = fm.lib()
    lib = fm._lib
    buf = (C.c_double * 64)()
    ptr = C.cast(buf, C.c_void_p)
    nan, inf = float("nan"), float("inf")

    def call(sp=True, xP=True, cones=True, left=True, right=True, n_left=4, n_right=4, per=0, P=1, N_w=8, Ltrack=100.0, margin=0.5, reach=5.0,
             n_lo=True, n_hi=True, M=100, dl=1.0):
        s = lib.Spline(M, dl, ptr if xP else None, ptr)
        c = lib.ConeMaps(ptr if left else None, ptr if right else None, n_left, n_right, per)
        return L.fsaempc_corridor_from_cones_device(C.byref(s) if sp else None, C.c_double(Ltrack), C.byref(c) if cones else None, P, N_w,
                                                    C.c_double(margin), C.c_double(reach), ptr if n_lo else None, ptr if n_hi else None, None, None)

    cases = [
        (dict(sp=False), -1, "cones: sp is NULL"),
        (dict(xP=False), -1, "cones: the spline tables are NULL"),
        (dict(cones=False), -1, "cones: cones is NULL"),
        (dict(n_lo=False), -1, "cones: n_lo is NULL"),
        (dict(n_hi=False), -1, "cones: n_hi is NULL"),
        (dict(P=0), -1, "cones: n_corridors must be >= 1"),
        (dict(N_w=1), -1, "cones: N_w must be >= 2"),
        (dict(Ltrack=0.0), -1, "cones: L must be finite and > 0"),
        (dict(Ltrack=nan), -1, "cones: L must be finite and > 0"),
        (dict(Ltrack=inf), -1, "cones: L must be finite and > 0"),
        (dict(margin=-0.1), -1, "cones: margin must be finite and >= 0"),
        (dict(margin=nan), -1, "cones: margin must be finite and >= 0"),
        (dict(margin=inf), -1, "cones: margin must be finite and >= 0"),
        (dict(reach=0.0), -1, "cones: reach must be finite and > 0"),
        (dict(reach=nan), -1, "cones: reach must be finite and > 0"),
        (dict(reach=inf), -1, "cones: reach must be finite and > 0"),
        (dict(n_left=-1), -1, "cones: n_left must be >= 0"),
        (dict(n_right=-1), -1, "cones: n_right must be >= 0"),
        (dict(left=False), -1, "cones: left is NULL with n_left > 0"),
        (dict(right=False), -1, "cones: right is NULL with n_right > 0"),
        (dict(M=0), -1, "cones: the spline needs M >= 1 and dl finite and > 0"),
        (dict(dl=nan), -1, "cones: the spline needs M >= 1 and dl finite and > 0"),
        (dict(n_left=513), -2, "cones: n_left exceeds FSAEMPC_CONES_MAX"),
        (dict(n_right=513), -2, "cones: n_right exceeds FSAEMPC_CONES_MAX"),
        (dict(M=513), -2, "cones: M exceeds FSAEMPC_CONES_MAX_M"),
    ]
    for kw, code, text in cases:
        assert call(**kw) == code, kw
        assert L.fsaempc_last_error().decode() == text, kw
    import torch
    if not torch.cuda.is_available():
        for kw in (dict(), dict(left=False, n_left=0), dict(right=False, n_right=0), dict(n_left=512, n_right=512, M=512), dict(margin=0.0, per=1)):
            assert call(**kw) == -4, (kw, L.fsaempc_last_error().decode())      # FSAEMPC_ERR_NODEVICE: nothing was refused
    hdr = open(os.path.join(ROOT, "include", "fsaempc.h")).read()
    assert "#define FSAEMPC_NCONEINFO 8" in hdr and "#define FSAEMPC_CONES_MAX 512" in hdr and "#define FSAEMPC_CONES_MAX_M 512" in hdr
    assert lib.NCONEINFO == cq.NCONEINFO == 8 and lib.CONES_MAX == cq.CONES_MAX == 512 and lib.CONES_MAX_M == cq.CONES_MAX_M == 512
    assert len(lib.CONE_INFO_INDEX) == 8


def test_the_python_mirror_of_the_cone_maps_matches_the_header(tmp_path):
    import subprocess
    import fsae_mpc_amd as fm
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fsaempc.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(fsaempc_cones), offsetof(fsaempc_cones, left), offsetof(fsaempc_cones, right),\n'
                   '         offsetof(fsaempc_cones, n_left), offsetof(fsaempc_cones, n_right), offsetof(fsaempc_cones, per_corridor));\n  return 0;\n}\n')
    exe = tmp_path / "s"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    M = fm._lib.ConeMaps
    assert got == [C.sizeof(M), M.left.offset, M.right.offset, M.n_left.offset, M.n_right.offset, M.per_corridor.offset]


def test_from_cones_refuses_bad_shapes_before_the_library():
    import fsae_mpc_amd as fm
    tr = fm.Track.load("fsg2019")
    ok = np.zeros((4, 2))
    for kw, word in ((dict(left=np.zeros((4, 3)), right=ok, N_w=8), "left must be"), (dict(left=ok, right=np.zeros(4), N_w=8), "right must be"),
                     (dict(left=ok, right=ok, N_w=1), "N_w"), (dict(left=np.zeros((513, 2)), right=ok, N_w=8), "at most 512"),
                     (dict(left=np.zeros((2, 4, 2)), right=np.zeros((3, 4, 2)), N_w=8), "different numbers of maps")):
        with pytest.raises(ValueError, match=word):
            fm.Corridor.from_cones(tr, device="cpu", **kw)


# ---- 6. cone_draws -------------------------------------------------------------------------------------------------------------------
def test_cone_draws():
    import fsae_mpc_amd as fm
    left, right = cone_maps()["fsg2019"]
    a, b = fm.cone_draws(left, right, 0.05, 8, 7)
    assert a.shape == (8,) + left.shape and b.shape == (8,) + right.shape
    a2, b2 = fm.cone_draws(left, right, 0.05, 8, 7)
    assert a.tobytes() == a2.tobytes() and b.tobytes() == b2.tobytes()                # reproducible by seed
    a3, _ = fm.cone_draws(left, right, 0.05, 8, 8)
    assert np.abs(a3 - a).max() > 1e-3                                                # another seed, other maps
    a4, _ = fm.cone_draws(left, right, 0.05, 3, 7)
    assert a4.tobytes() == a[:3].tobytes()                                            # copy p does not depend on P
    assert np.abs(a[0] - a[1]).max() > 1e-3 and np.abs(a - left).max() < 0.05 * 6
    sd = np.concatenate([(a - left).ravel(), (b - right).ravel()]).std()
    assert 0.045 < sd < 0.055, sd                                                     # 2464 draws: 0.05 +- 3 * 0.05 / sqrt(2 * 2464)
    z, y = fm.cone_draws(left, right, 0.0, 4, 7)
    assert all(z[p].tobytes() == np.ascontiguousarray(left).tobytes() and y[p].tobytes() == np.ascontiguousarray(right).tobytes() for p in range(4))
    with pytest.raises(ValueError):
        fm.cone_draws(left, right, -1.0, 4, 7)
    with pytest.raises(ValueError):
        fm.cone_draws(left, right, 0.1, 0, 7)
