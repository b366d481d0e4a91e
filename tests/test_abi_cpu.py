"""CPU tests of the product's host side: the C-ABI library loads and exports every symbol include/fsaempc.h
declares (no compute without a GPU), argument validation mirrors the MEX gateway, host-side generators agree
with the oracle's, and the N>1 sharding/gather path works over gloo."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_library_exports_every_declared_symbol():
    import fsae_mpc_amd as fm
    hdr = open(os.path.join(ROOT, "include", "fsaempc.h")).read()
    declared = set(re.findall(r"\b(fsaempc_[A-Za-z_0-9]+)\s*\(", hdr))
    declared -= {"fsaempc_qp_opts", "fsaempc_qp_desc", "fsaempc_spline", "fsaempc_ltv_desc"}
    assert declared == set(fm._lib.EXPORTS)
    L = fm.lib()
    for s in sorted(declared):
        assert hasattr(L, s), s


def test_default_opts_and_dims():
    import fsae_mpc_amd as fm
    o = fm.default_opts()
    assert o.tol == 1e-8 and o.tol_loose == 1e-6 and o.inf_bound == 1e9 and o.max_iter == 100 and o.polish == 1
    assert fm.dims(fm.KINEMATIC, 40) == (5, 1, 81, 240) and fm.dims(fm.DYNAMIC, 60) == (7, 4, 124, 1200)
    d = fm._lib.QpDesc(81, 240, 4096, 0)
    assert fm.lib().fsaempc_qp_workspace_bytes(C.byref(d)) > 4096 * 240 * 81 * 8
    d = fm._lib.QpDesc(200, 10, 1, 0)
    assert fm.lib().fsaempc_qp_workspace_bytes(C.byref(d)) == -2   # FSAEMPC_ERR_DIM


def test_struct_layouts_of_the_python_mirror_match_the_header(tmp_path):
    """The ctypes structures of fsae-mpc_amd/_lib.py against include/fsaempc.h: sizes and member offsets as the C compiler sees them
    (a field added to one side only -- fsaempc_qp_aux.x_init and .difficulty came in round 3 -- would silently shift every later member)."""
    import subprocess, ctypes as C
    from fsae_mpc_amd import _lib
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    src = tmp_path / "layout.c"
    src.write_text("""
#include <stdio.h>
#include <stddef.h>
#include "fsaempc.h"
int main(void) {
  printf("aux %zu %zu %zu %zu %zu\\n", sizeof(fsaempc_qp_aux), offsetof(fsaempc_qp_aux, kkt), offsetof(fsaempc_qp_aux, polished), offsetof(fsaempc_qp_aux, x_init), offsetof(fsaempc_qp_aux, difficulty));
  printf("desc %zu %zu %zu %zu %zu\\n", sizeof(fsaempc_qp_desc), offsetof(fsaempc_qp_desc, nV), offsetof(fsaempc_qp_desc, nC), offsetof(fsaempc_qp_desc, batch), offsetof(fsaempc_qp_desc, shared_HA));
  printf("opts %zu %zu %zu\\n", sizeof(fsaempc_qp_opts), offsetof(fsaempc_qp_opts, max_iter), offsetof(fsaempc_qp_opts, polish));
  return 0;
}
""".replace("\\\\n", "\\n"))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    out = dict((l.split()[0], [int(v) for v in l.split()[1:]]) for l in subprocess.check_output([str(exe)], text=True).splitlines())
    A, D = _lib.QpAux, _lib.QpDesc
    assert out["aux"] == [C.sizeof(A), A.kkt.offset, A.polished.offset, A.x_init.offset, A.difficulty.offset], out["aux"]
    assert out["desc"] == [C.sizeof(D), D.nV.offset, D.nC.offset, D.batch.offset, D.shared_HA.offset], out["desc"]
    O = type(_lib.default_opts()) if hasattr(_lib, "default_opts") else None
    if O is not None:
        assert out["opts"] == [C.sizeof(O), O.max_iter.offset, O.polish.offset], out["opts"]


def test_gateway_argument_validation():
    import fsae_mpc_amd as fm
    H = np.eye(2); g = np.zeros(2)
    with pytest.raises(fm.FsaempcError, match="NaN"):
        fm.qpOASES(H, np.array([np.nan, 0]), [0, 0], [1, 1])
    with pytest.raises(ValueError, match="dimension mismatch"):
        fm.qpOASES(H, g, np.ones((1, 3)), [0, 0], [1, 1], [0], [1])
    with pytest.raises(TypeError):
        fm.qpOASES(H, g, [0, 0])


def test_sequence_handle_errors():
    import fsae_mpc_amd as fm
    # main.m:193 calls qpOASES_sequence('c', QP) with QP == 0: the gateway answers "Invalid handle to QP instance!"
    with pytest.raises(fm.FsaempcError, match="Invalid handle"):
        fm.qpOASES_sequence("c", 0)
    with pytest.raises(fm.FsaempcError, match="Invalid handle"):
        fm.qpOASES_sequence("h", 7, [0.0], [0.0], [1.0], [], [])


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import fsae_mpc_amd as fm
    with pytest.raises(fm.FsaempcError):
        fm.qpOASES(np.eye(2), np.zeros(2), [0, 0], [1, 1])
    assert fm.lib().fsaempc_selftest_mfma() < 0


def test_product_generators_match_oracle(orc, otrack):
    import fsae_mpc_amd as fm
    tr = fm.Track.load("fsg2019")
    assert tr.M == otrack.M and tr.dl == otrack.dl and np.array_equal(tr.xP, otrack.xP)
    for model in (fm.KINEMATIC, fm.DYNAMIC):
        a = fm.instances(model, 12, 0.05, tr.L, 20190, np.arange(100, 164))
        b = orc.synth_instances(model, 12, 0.05, tr.L, 20190, np.arange(100, 164))
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


def _dist_worker(rank, world, port, q):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from fsae_mpc_amd import shard
    B = 37
    lo, hi = shard.shard_range(B, rank, world)
    local = torch.arange(lo, hi, dtype=torch.float64)[:, None] * torch.ones(1, 3, dtype=torch.float64)  # stand-in per-instance results
    full = shard.gather_rows(local, B, rank, world)
    ok = bool(torch.equal(full[:, 0], torch.arange(B, dtype=torch.float64)))
    tmax = shard.max_over_ranks(float(rank + 1))
    # the packed result block of the bench's gather: (B/G) x (nV + 2) doubles per rank, one all_gather_into_tensor
    per, nV = 6, 5
    rg = shard.ResultGather(per, nV, world, "cpu")
    ids = torch.arange(rank * per, (rank + 1) * per, dtype=torch.float64)
    x = ids[:, None] + torch.arange(nV, dtype=torch.float64)[None, :] / 16.0
    fl = torch.tensor([0, 1, -1, -2, -3, 0], dtype=torch.int32); it = (torch.arange(per, dtype=torch.int32) * 37 + rank) % 1024
    send_ptr, recv_ptr = rg.send.data_ptr(), rg.recv.data_ptr()
    for _ in range(2):                                   # reused across steps: same buffers
        rg.pack(x, ids * 0.5, fl, it)
        blk = rg.gather()
    gx, gf, gfl, git = shard.ResultGather.unpack(blk, nV)
    allids = torch.arange(world * per, dtype=torch.float64)
    ok = ok and rg.send.data_ptr() == send_ptr and rg.recv.data_ptr() == recv_ptr and blk.shape == (world * per, nV + 2)
    ok = ok and bool(torch.equal(gx, allids[:, None] + torch.arange(nV, dtype=torch.float64)[None, :] / 16.0)) and bool(torch.equal(gf, allids * 0.5))
    ok = ok and bool(torch.equal(gfl, fl.repeat(world))) and bool(torch.equal(git, torch.cat([(torch.arange(per, dtype=torch.int32) * 37 + r) % 1024 for r in range(world)])))
    q.put((rank, lo, hi, ok, tmax))
    dist.destroy_process_group()


def test_sharding_and_gather_over_gloo():
    import torch.multiprocessing as mp
    import fsae_mpc_amd  # noqa: F401
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + os.getpid() % 2000
    ps = [ctx.Process(target=_dist_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps: p.start()
    res = sorted(q.get(timeout=120) for _ in ps)
    for p in ps: p.join(60)
    assert res[0][1:3] == (0, 19) and res[1][1:3] == (19, 37)
    assert all(r[3] for r in res) and all(r[4] == 2.0 for r in res)


def test_bench_self_starts_two_ranks_over_gloo():
    """`python bench.py --gpus 2` with no launcher around it starts its own ranks: the dry run takes the same
    launch -> init_process_group -> shard -> gather_rows -> max_over_ranks -> one JSON line route as the GPU run, on gloo."""
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run", "--batch", "37", "--steps", "2", "--warmup", "0"],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout                      # exactly one JSON line, from rank 0
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 2 and out["scaling"] == "weak"
    assert out["config"]["gathered_rows"] == 74 and out["config"]["gather_ok"]
    for k in ("metric", "value", "unit", "ms_per_step", "higher_is_better", "vs_baseline", "dtype", "data", "roofline", "cpu_baseline"):
        assert k in out


def test_bench_dump_outputs_float64_and_bounded(tmp_path):
    """bench.py --dump-outputs: every array as float64 (exit flags / iteration counts exact); above 64 MB in all, one fixed, seeded
    sample of instances taken from every array alike, with its row ids"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    small = tmp_path / "small"
    bench.dump_outputs(str(small), dict(x=np.arange(12.0).reshape(4, 3), exitflag=np.array([0, 1, -1, 0], dtype=np.int32)))
    assert sorted(os.listdir(small)) == ["exitflag.npy", "x.npy"]
    fl = np.load(small / "exitflag.npy")
    assert fl.dtype == np.float64 and np.array_equal(fl, [0, 1, -1, 0])
    B, nV = 70000, 124
    x = np.arange(B, dtype=np.float64)[:, None] * np.ones(nV)
    dirs = [tmp_path / "big1", tmp_path / "big2"]
    for d in dirs:
        bench.dump_outputs(str(d), dict(x=x, iter=np.arange(B, dtype=np.int32)))
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64 << 20
    rows = np.load(dirs[0] / "sample_rows.npy")
    assert np.array_equal(rows, np.load(dirs[1] / "sample_rows.npy")) and np.all(np.diff(rows) > 0)
    assert np.array_equal(np.load(dirs[0] / "x.npy")[:, 0], rows) and np.array_equal(np.load(dirs[0] / "iter.npy"), rows)


@pytest.mark.parametrize("src", ["qpOASES.cpp", "qpOASES_sequence.cpp"])
def test_mex_gateways_compile(src):
    """the MEX gateways type-check against a stand-in mex.h and the real include/fsaempc.h (no MATLAB in this image)"""
    import subprocess
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "tests", "stub_mex"),
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "mex", src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_mex_gateways_run(tmp_path):
    """Both MEX gateways RUN on the CPU against a functional stand-in of the MEX API (tests/stub_mex/mex_fake.cpp) and a recording
    stand-in of libfsaempc (tests/stub_mex/run_gateways.cpp): every call form of qpOASES.m:22-23,34-35,65-67 and
    qpOASES_sequence.m:23-26,39-42,51,64,76 -- general and bounds-only, k columns, options, auxInput, auxOutput -- must hand each
    argument to the right position of the C ABI (sentinel values) and lay the outputs out in the reference's order."""
    import subprocess
    d = os.path.join(ROOT, "tests", "stub_mex")
    exe = str(tmp_path / "run_gateways")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + d, "-I" + os.path.join(ROOT, "include"), os.path.join(d, "run_gateways.cpp"),
                        os.path.join(d, "mex_fake.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "gateways ok" in r.stdout, r.stdout + r.stderr


# ---- track pipeline as a library: csrc/track.cpp through the C ABI, host side only -----------------------------
def _py_tool():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_track_tables", os.path.join(ROOT, "tools", "make_track_tables.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("shape", ["circle", "oval", "kidney"])
def test_track_library_vs_numpy_restatement_known_tracks(tmp_path, shape):
    """Library (C++: cyclic solve, own Gauss-Kronrod quadrature, bisection) against the numpy / scipy restatement of the same
    three reference files (tools/make_track_tables.py: dense solve, QUADPACK) on synthetic closed tracks written as race-line CSVs
    in the reference's format, to 1e-9 -- plus what any such table must satisfy: M * dl = L, C1 / C2 joins of the periodic
    Bezier spline, and for the circle the stations' distance from the centre."""
    import fsae_mpc_amd as fm
    tool = _py_tool()
    n = {"circle": 60, "oval": 90, "kidney": 120}[shape]
    th = np.linspace(0, 2 * np.pi, n, endpoint=False) + 0.1234   # (no symmetry: a station that falls exactly on a knot of the input spline
    #  makes `find(l_cum >= i*dl, 1)` a coin toss of the last bit, and the 0.01 bisection then stops elsewhere)
    if shape == "circle":
        x, y = 30 * np.cos(th), 30 * np.sin(th)
    elif shape == "oval":
        x, y = 60 * np.cos(th), 25 * np.sin(th)
    else:
        r = 40 + 12 * np.cos(2 * th) + 5 * np.sin(3 * th)
        x, y = r * np.cos(th), r * np.sin(th)
    csv = tmp_path / (shape + ".csv")
    with open(csv, "w") as f:
        f.write("X,Y,vX,vY,aX,aY,dt,rX,rY,lX,lY\n")
        for a, b in zip(x, y):
            f.write("%.17g,%.17g,0,0,0,0,0.1,0,0,0,0\n" % (a, b))
    M = 100
    tr = fm.Track.from_csv(str(csv), M)
    xs, ys = tool.make_spline_periodic(x), tool.make_spline_periodic(y)
    xP, yP, dl, L = tool.arclength_reparam(xs, ys, M)
    assert abs(tr.dl - dl) <= 1e-9 * dl and abs(tr.L - L) <= 1e-9 * L and abs(M * tr.dl - tr.L) <= 1e-12 * tr.L
    assert np.abs(tr.xP - xP).max() <= 1e-9 * np.abs(xP).max() and np.abs(tr.yP - yP).max() <= 1e-9 * np.abs(yP).max()
    for P in (tr.xP, tr.yP):
        Pn = np.roll(P, -1, axis=0)
        assert np.abs(P[:, 3] - Pn[:, 0]).max() <= 1e-12 * np.abs(P).max()                                   # C0
        assert np.abs((P[:, 3] - P[:, 2]) - (Pn[:, 1] - Pn[:, 0])).max() <= 1e-9 * np.abs(P).max()           # C1
        assert np.abs((P[:, 3] - 2 * P[:, 2] + P[:, 1]) - (Pn[:, 2] - 2 * Pn[:, 1] + Pn[:, 0])).max() <= 1e-9 * np.abs(P).max()   # C2
    if shape == "circle":
        # the M stations lie on the input spline, i.e. on the circle up to its fit error.  (Their spacing is NOT uniform: the
        # reference's speed integrand starts every segment at zero, arclength_reparam.m:20-23 -- the quirk is kept, so curvature
        # read off this table is only as good as the reference's own.)
        assert np.abs(np.hypot(tr.xP[:, 0], tr.yP[:, 0]) - 30.0).max() <= 1e-3 * 30.0
    # table file round trip (FSTRK001)
    path = str(tmp_path / "t.fstrk")
    tr.save_table(path)
    tr2 = fm.Track.load_table(path)
    assert tr2.M == M and tr2.dl == tr.dl and tr2.L == tr.L and np.array_equal(tr2.xP, tr.xP) and np.array_equal(tr2.yP, tr.yP)


@pytest.mark.parametrize("name", ["fsg2019", "fss2019", "fso2020"])
def test_track_library_reproduces_the_committed_tables(tmp_path, name):
    """The committed tables (fsae-mpc_amd/tracks/*.json, made by tools/make_track_tables.py from the reference's CSVs) against the
    library run on the same race line.  The race lines' X, Y columns (all the reader uses) are stored in
    tests/golden/tracks/raceline_xy.npz and written back as a CSV in the reference's format (%.17g: the same doubles)."""
    import fsae_mpc_amd as fm
    z = np.load(os.path.join(ROOT, "tests", "golden", "tracks", "raceline_xy.npz"))
    csv = tmp_path / (name + ".csv")
    with open(csv, "w") as f:
        f.write("X,Y,vX,vY,aX,aY,dt,rX,rY,lX,lY\n")
        for a, b in zip(z[name + "_x"], z[name + "_y"]):
            f.write("%.17g,%.17g,0,0,0,0,0.1,0,0,0,0\n" % (a, b))
    tr, ref = fm.Track.from_csv(str(csv), 100), fm.Track.load(name)
    assert abs(tr.dl - ref.dl) <= 1e-9 * ref.dl and abs(tr.L - ref.L) <= 1e-9 * ref.L
    assert np.abs(tr.xP - ref.xP).max() <= 1e-9 * np.abs(ref.xP).max() and np.abs(tr.yP - ref.yP).max() <= 1e-9 * np.abs(ref.yP).max()


def test_track_library_rejects_bad_input(tmp_path):
    import fsae_mpc_amd as fm
    with pytest.raises(fm.FsaempcError, match="cannot open"):
        fm.Track.from_csv(str(tmp_path / "missing.csv"))
    p = tmp_path / "short.csv"
    p.write_text("X,Y\n1,2\n3,4\n")
    with pytest.raises(fm.FsaempcError, match="fewer than three"):
        fm.Track.from_csv(str(p))
    with pytest.raises(fm.FsaempcError, match="not an FSTRK001"):
        fm.Track.load_table(str(p))
