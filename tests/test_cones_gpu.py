"""GPU tests of the corridors from cone positions: cor_from_cones_kernel against the brute-force ray cast and the numpy
restatement (tests/cones_numpy.py), the known answer, batches and cone order, the sizes at which the kernel takes another path, and
the corridor's way into the MPC step, the racing line and the per-car Monte-Carlo.  The comparison tolerance is the project's
construction tolerance (BUILD_TOL of tests/test_corridor_gpu.py) through conftest.relerr."""
import numpy as np
import pytest
from conftest import relerr

import cones_numpy as cq
import corridor_numpy as cn
from cones_cases import MARGIN, REACH, TRACKS, cone_maps, insert_on_chords, known_answer_cones, reference_case

pytestmark = pytest.mark.gpu

BUILD_TOL = 1e-9        # the project's construction tolerance
DT = 0.05


@pytest.fixture(scope="module")
def fm():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import fsae_mpc_amd
    return fsae_mpc_amd


@pytest.fixture(scope="module")
def torch_():
    import torch
    return torch


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _np(torch, d):
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in d.items()}


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _tables(cor):
    return cor.n_lo.cpu().numpy(), cor.n_hi.cpu().numpy()


def _raw(fm, torch, tr, left, right, N_w, margin, reach=REACH):
    """The C entry itself for one corridor, whatever its info says: (n_lo (N_w,), n_hi (N_w,), info (8,))"""
    import ctypes as C
    le, ri = _dev(torch, np.asarray(left).reshape(-1, 2)), _dev(torch, np.asarray(right).reshape(-1, 2))
    xP, yP = tr.device("cuda:0")
    sp = fm._lib.Spline(tr.M, tr.dl, C.c_void_p(xP.data_ptr()), C.c_void_p(yP.data_ptr()))
    maps = fm._lib.ConeMaps(C.c_void_p(le.data_ptr() if le.numel() else None), C.c_void_p(ri.data_ptr() if ri.numel() else None),
                            le.shape[0], ri.shape[0], 0)
    out = torch.full((2 * N_w + 8,), -7.0, dtype=torch.float64, device="cuda")
    rc = fm.lib().fsaempc_corridor_from_cones_device(C.byref(sp), C.c_double(tr.L), C.byref(maps), 1, N_w, C.c_double(margin), C.c_double(reach),
                                                     C.c_void_p(out.data_ptr()), C.c_void_p(out.data_ptr() + 8 * N_w),
                                                     C.c_void_p(out.data_ptr() + 16 * N_w), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, fm.lib().fsaempc_last_error()
    h = out.cpu().numpy()
    return h[:N_w], h[N_w:2 * N_w], h[2 * N_w:]


# ---- 1. parity -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TRACKS)
def test_1_parity_with_the_ray_cast_and_the_restatement(fm, name):
    N_w = 64
    tr, left, right, lo, hi, inf = reference_case(name, N_w)
    cor = fm.Corridor.from_cones(tr, left, right, N_w, margin=MARGIN, reach=REACH)
    assert cor.P == 1 and cor.N_w == N_w and cor.L == tr.L and cor.info.shape == (1, 8)
    glo, ghi = _tables(cor)
    el, _ = cq.ray_cast(tr, tr.L, left, N_w, +1, REACH)
    er, _ = cq.ray_cast(tr, tr.L, right, N_w, -1, REACH)
    errs = (relerr(ghi[0], el - MARGIN), relerr(glo[0], er + MARGIN), relerr(ghi[0], hi), relerr(glo[0], lo))
    print(name, "ray cast: n_hi %.3e n_lo %.3e; restatement: n_hi %.3e n_lo %.3e; info" % errs, cor.info[0])
    assert max(errs) <= BUILD_TOL, errs
    assert cor.info[0, 0] == len(left) and cor.info[0, 1] == len(right)
    assert (cor.info[0, 2:7] == 0).all(), cor.info[0]
    assert abs(cor.info[0, 7] - inf[7]) <= 1e-9
    assert cor.info[0, 7] == (ghi[0] - glo[0]).min()


# ---- 2. known answer -----------------------------------------------------------------------------------------------------------------
def test_2_known_answer(fm):
    tr = fm.Track.load("fsg2019")
    N_w, K, margin = 64, 32, 0.1      # (the cones are 0.5 .. 1.5 m from the line: the margin leaves every cell room)
    cells, cl, wl = known_answer_cones(tr, N_w, K, +1)
    _, cr, wr = known_answer_cones(tr, N_w, K, -1)
    assert len(cells) == K
    cor = fm.Corridor.from_cones(tr, cl, cr, N_w, margin=margin, reach=REACH)
    lo, hi = _tables(cor)
    eh, el = np.abs(hi[0, cells] - (wl - margin)).max(), np.abs(lo[0, cells] - (wr + margin)).max()
    print("known answer: n_hi", eh, "n_lo", el, cor.info[0])
    assert eh <= 1e-9 and el <= 1e-9
    assert cor.info[0, 0] == K and cor.info[0, 1] == K and (cor.info[0, 2:5] == 0).all() and cor.info[0, 6] == 0


# ---- 3. batch and order --------------------------------------------------------------------------------------------------------------
def test_3_batch_order_padding_and_strays(fm):
    N_w = 64
    tr, left, right, lo, hi, _ = reference_case("fsg2019", N_w)
    Kl, Kr, pad = len(left), len(right), 5
    far = np.array([[left[:, 0].max() + 50.0, left[:, 1].max() + 50.0]])     # a stray: 50 m outside the box round the track
    nanrow = np.full((pad - 1, 2), np.nan)
    fill = lambda a: np.concatenate([a, np.full((pad, 2), np.nan)])
    maps_l = np.stack([fill(left), fill(left[np.random.default_rng(3).permutation(Kl)]), np.concatenate([left[:10], nanrow, left[10:], far])])
    maps_r = np.stack([fill(right), fill(right[np.random.default_rng(4).permutation(Kr)]), np.concatenate([far, right[:40], nanrow, right[40:]])])
    cor = fm.Corridor.from_cones(tr, maps_l, maps_r, N_w, margin=MARGIN, reach=REACH)
    assert cor.P == 3
    glo, ghi = _tables(cor)
    for p in (1, 2):
        assert _same_bits(glo[p], glo[0]) and _same_bits(ghi[p], ghi[0]), p
    assert relerr(glo[0], lo) <= BUILD_TOL and relerr(ghi[0], hi) <= BUILD_TOL
    for p in range(3):                                                  # each equals its own call
        one = fm.Corridor.from_cones(tr, maps_l[p], maps_r[p], N_w, margin=MARGIN, reach=REACH)
        olo, ohi = _tables(one)
        assert _same_bits(olo[0], glo[p]) and _same_bits(ohi[0], ghi[p]) and _same_bits(one.info[0], cor.info[p]), p
    import torch
    dev = fm.Corridor.from_cones(tr, _dev(torch, maps_l), _dev(torch, maps_r), N_w, margin=MARGIN, reach=REACH)   # maps already on the device
    dlo, dhi = _tables(dev)
    assert _same_bits(dlo, glo) and _same_bits(dhi, ghi) and _same_bits(dev.info, cor.info)
    plain = fm.Corridor.from_cones(tr, left, right, N_w, margin=MARGIN, reach=REACH)      # the maps without any padding
    plo, phi = _tables(plain)
    assert _same_bits(plo[0], glo[0]) and _same_bits(phi[0], ghi[0])
    assert (cor.info[:, 0] == Kl).all() and (cor.info[:, 1] == Kr).all()
    assert cor.info[:, 2].tolist() == [2 * pad, 2 * pad, 2 * (pad - 1)] and cor.info[:, 4].tolist() == [0, 0, 2], cor.info
    assert (cor.info[:, 3] == 0).all() and (cor.info[:, 5:7] == 0).all()


# ---- 4. sizes ------------------------------------------------------------------------------------------------------------------------
def test_4_one_and_two_cones(fm, torch_):
    """K = 1: a constant table.  K = 2: two chords of half a lap each, so most cells take the safeguards (the clamp, the arc-length
    form of t) and many have no room -- the tables and the counts are the restatement's all the same."""
    tr = fm.Track.load("fsg2019")
    N_w = 64
    for K in (1, 2):
        cells, cl, wl = known_answer_cones(tr, N_w, K, +1)
        _, cr, wr = known_answer_cones(tr, N_w, K, -1)
        lo, hi, info = _raw(fm, torch_, tr, cl, cr, N_w, 0.25)
        wlo, whi, winf = cq.corridor_from_cones(tr, tr.L, cl, cr, N_w, 0.25, REACH)
        print("K =", K, "info", info, "restatement", winf)
        assert info[0] == K and info[1] == K
        assert relerr(lo, wlo) <= BUILD_TOL and relerr(hi, whi) <= BUILD_TOL, K
        assert np.array_equal(info[:7], winf[:7]) and abs(info[7] - winf[7]) <= 1e-9, (info, winf)
        assert np.abs(hi[cells] - (wl - 0.25)).max() <= 1e-9 and np.abs(lo[cells] - (wr + 0.25)).max() <= 1e-9
        if K == 1:
            assert (hi == hi[0]).all() and (lo == lo[0]).all()
            cor = fm.Corridor.from_cones(tr, cl, cr, N_w, margin=0.25)
            assert _same_bits(cor.n_hi.cpu().numpy()[0], hi) and _same_bits(cor.info[0], info)


def test_4_more_cones_than_threads(fm):
    """fss2019 (83 cones per side) with two and with three points inserted on every chord: 249 per side (sort size 256, nearly every
    thread busy) and 332 per side (more cones than threads, sort size 512).  Points on a chord leave the polyline as it is, so the
    tables are those of the K = 83 call."""
    N_w = 64
    tr, left, right, lo, hi, _ = reference_case("fss2019", N_w)
    base = fm.Corridor.from_cones(tr, left, right, N_w, margin=MARGIN, reach=REACH)
    blo, bhi = _tables(base)
    for m in (2, 3):
        l2, r2 = insert_on_chords(left, m), insert_on_chords(right, m)
        assert len(l2) == (m + 1) * 83
        cor = fm.Corridor.from_cones(tr, l2, r2, N_w, margin=MARGIN, reach=REACH)
        glo, ghi = _tables(cor)
        errs = (relerr(glo[0], blo[0]), relerr(ghi[0], bhi[0]), relerr(glo[0], lo), relerr(ghi[0], hi))
        print("inserted", m, "K =", len(l2), errs, cor.info[0])
        assert max(errs) <= BUILD_TOL, (m, errs)
        assert cor.info[0, 0] == len(l2) and cor.info[0, 1] == len(r2) and (cor.info[0, 2:7] == 0).all()


def test_4_a_side_without_cones(fm, torch_):
    N_w = 64
    tr, left, right, lo, hi, _ = reference_case("fsg2019", N_w)
    none = np.zeros((0, 2))
    with pytest.raises(ValueError, match="corridor 0: no right cone"):
        fm.Corridor.from_cones(tr, left, none, N_w, margin=MARGIN)
    with pytest.raises(ValueError, match="corridor 0: no left cone"):
        fm.Corridor.from_cones(tr, np.full((4, 2), np.nan), right, N_w, margin=MARGIN)
    cor = fm.Corridor.from_cones(tr, left, none, N_w, margin=MARGIN, check=False)
    assert cor.info is None
    glo, ghi = _tables(cor)
    assert np.isnan(glo).all() and relerr(ghi[0], hi) <= BUILD_TOL
    # the info of such a call, from the C entry itself: kept = 0 on the right, every cell counted, no least width
    rlo, rhi, got = _raw(fm, torch_, tr, left, none, N_w, MARGIN)
    assert np.isnan(rlo).all() and _same_bits(rhi, ghi[0])
    assert got[0] == len(left) and got[1] == 0 and (got[2:6] == 0).all() and got[6] == N_w and np.isnan(got[7]), got
    # a cell without room (the margin is wider than the track) is named too
    with pytest.raises(ValueError, match="n_lo < n_hi fails"):
        fm.Corridor.from_cones(tr, left, right, N_w, margin=2.5)


@pytest.mark.parametrize("N_w", [2, 1000])
def test_4_fewest_cells_and_more_cells_than_threads(fm, N_w):
    tr, left, right, lo, hi, inf = reference_case("fsg2019", N_w)
    cor = fm.Corridor.from_cones(tr, left, right, N_w, margin=MARGIN, reach=REACH)
    glo, ghi = _tables(cor)
    assert relerr(glo[0], lo) <= BUILD_TOL and relerr(ghi[0], hi) <= BUILD_TOL
    assert np.array_equal(cor.info[0, :7], inf[:7]) and abs(cor.info[0, 7] - inf[7]) <= 1e-9


# ---- 5. plumbing ---------------------------------------------------------------------------------------------------------------------
def test_5_the_mpc_step_reads_the_tables_where_they_are(fm, torch_):
    torch = torch_
    tr, left, right, _, _, _ = reference_case("fsg2019", 64)
    model, N, B = fm.KINEMATIC, 5, 4
    cor = fm.Corridor.from_cones(tr, left, right, 64, margin=MARGIN)
    lo, hi = _tables(cor)
    copy = fm.Corridor.from_table(lo[0], hi[0], tr.L)
    x0, xl, ul, xr = fm.instances(model, N, DT, tr.L, 31, range(B))
    inp = lambda: (_dev(torch, x0), _dev(torch, xr), _dev(torch, xl), _dev(torch, ul))
    for what in ("build_qp", "step"):
        a = _np(torch, getattr(fm.LtvBatch(model, N, DT, tr, B, corridor=cor), what)(*inp()))
        b = _np(torch, getattr(fm.LtvBatch(model, N, DT, tr, B, corridor=copy), what)(*inp()))
        assert set(a) == set(b)
        for k in a:
            if isinstance(a[k], np.ndarray):
                assert _same_bits(a[k], b[k]), (what, k)
        if what == "build_qp":                                                            # (the corridor is not the band)
            plain = _np(torch, fm.LtvBatch(model, N, DT, tr, B).build_qp(*inp()))
            assert np.abs(a["ubA"][:, 3 * N:4 * N] - plain["ubA"][:, 3 * N:4 * N]).min() > 0.1
    assert (a["exitflag"] == 0).all(), a["exitflag"]


def test_5_the_racing_line_reads_the_tables_where_they_are(fm, torch_):
    torch = torch_
    tr, left, right, _, _, _ = reference_case("fsg2019", 64)
    cor = fm.Corridor.from_cones(tr, left, right, 64, margin=MARGIN)
    lo, hi = _tables(cor)
    copy = fm.Corridor.from_table(lo[0], hi[0], tr.L)
    pa = fm.Plan.raceline(fm.KINEMATIC, tr, N_s=64, N_c=16, margin=0.1, corridor=cor, rows="cells")
    pb = fm.Plan.raceline(fm.KINEMATIC, tr, N_s=64, N_c=16, margin=0.1, corridor=copy, rows="cells")
    torch.cuda.synchronize()
    print("line QP flags in the cone corridor:", pa.line_flag.cpu().numpy())
    for k in ("line", "line_flag", "table", "t"):
        assert _same_bits(getattr(pa, k).cpu().numpy(), getattr(pb, k).cpu().numpy()), k


# ---- 6. a per-car Monte-Carlo --------------------------------------------------------------------------------------------------------
def test_6_every_car_drives_in_the_corridor_of_its_own_cone_map(fm, torch_):
    torch = torch_
    tr, left, right, _, _, _ = reference_case("fsg2019", 64)
    model, N, B, N_w = fm.KINEMATIC, 10, 8, 64
    dl, dr = fm.cone_draws(left, right, 0.05, B, 5)
    cor = fm.Corridor.from_cones(tr, dl, dr, N_w, margin=MARGIN)
    assert cor.P == B and (cor.info[:, 0] == len(left)).all() and (cor.info[:, 6] == 0).all()
    lo, hi = _tables(cor)
    assert np.abs(lo[0] - lo[7]).max() > 1e-3                                             # eight different corridors
    cl, flags, iters, active = fm.monte_carlo(model, N, tr, B, 3, corridor=cor, metrics=True)
    assert flags.shape == (3, B) and active[0].all()
    rep = cl.report()
    assert rep is not None
    q = _np(torch, cl.mpc.build_qp(cl.x0, cl.x_ref, cl.x_opt, cl.u_opt))                  # the QP of the next step, built by the loop's own MPC
    s_lin = cl.x_opt.cpu().numpy()[:, :, 0]
    pred_n = q["pred"].reshape(B, N, -1)[:, :, 1]
    for b in (0, 7):
        wl, wu = cn.row_bounds(lo[b], hi[b], tr.L / N_w, s_lin[b], pred_n[b])
        el, eu = np.abs(q["lbA"][b, 2 * N:3 * N] - wl).max(), np.abs(q["ubA"][b, 3 * N:4 * N] - wu).max()
        assert el <= BUILD_TOL and eu <= BUILD_TOL, (b, el, eu)
        other = 7 - b
        xl, xu = cn.row_bounds(lo[other], hi[other], tr.L / N_w, s_lin[b], pred_n[b])
        assert np.abs(q["lbA"][b, 2 * N:3 * N] - xl).max() > 1e-4                         # (and not the other car's)
