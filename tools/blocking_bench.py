#!/usr/bin/env python3
"""Move blocking on one MI355X: the fused step with held inputs next to the unblocked step of the same model, N and
batch, the two interleaved round-robin in one run -- phase times by the library's HIP events (fsaempc_ltv_get_timing), the median of
`steps` steps after `warmup` warm-up steps per variant, QP/s, mean interior-point iterations, non-zero exit flags and the share of
instances returned at the vertex.  Then a closed loop of 256 cars x 50 steps, blocked next to unblocked: the abnormal-exit tally,
the mean and median predicted cost of the solved steps (the mean is carried by the few steps that pay a 1e8 slack cost) and the mean realised lateral / heading cost of the cars still driving.

--parent-lib PATH: also measures the unblocked fused step of another build of the library (the parent commit's libfsaempc.so) in
the same session, in child processes before and after the interleaved run (a library is bound once per process); the verdict
`blocked_faster_than_parent` compares the blocked step with the faster of the two.  Without it the unblocked variant of this build,
the same code path, stands in.

usage: blocking_bench.py [out.json] [B=4096] [steps=30] [warmup=5] [--parent-lib PATH]"""
import ctypes as C, json, os, subprocess, sys
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import torch
import fsae_mpc_amd as fm
from fsae_mpc_amd import _lib

SHAPES = [(fm.DYNAMIC, 80, [2] * 40), (fm.DYNAMIC, 60, [2] * 30), (fm.KINEMATIC, 40, [2] * 20)]
argv = [a for a in sys.argv[1:]]
parent_lib = None
child_lib = None
for flag in ("--parent-lib", "--unblocked-with"):
    if flag in argv:
        i = argv.index(flag)
        if flag == "--parent-lib":
            parent_lib = os.path.abspath(argv[i + 1])
        else:
            child_lib = argv[i + 1]
        del argv[i:i + 2]
out_path = argv[0] if len(argv) > 0 else os.path.join(ROOT, "profiles", "blocking", "blocking_bench_B4096.json")
B = int(argv[1]) if len(argv) > 1 else 4096
steps = max(20, int(argv[2])) if len(argv) > 2 else 30
warmup = int(argv[3]) if len(argv) > 3 else 5
tr = fm.Track.load("fsg2019")
up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
name = lambda model: "dynamic" if model == fm.DYNAMIC else "kinematic"


def summary(rows):
    r = np.array(rows)
    return {"build_ms": float(np.median(r[:, 0])), "prep_ms": float(np.median(r[:, 1])), "solve_ms": float(np.median(r[:, 2])),
            "post_ms": float(np.median(r[:, 3])), "step_ms": float(np.median(r.sum(1))), "step_ms_min": float(r.sum(1).min()),
            "step_ms_max": float(r.sum(1).max()), "qp_per_s": float(B / np.median(r.sum(1)) * 1e3)}


def unblocked_with(path):
    """Child mode: the unblocked fused step of the library at `path` through its own symbols only (an older build has no blocked
    entries, so the package's binding is not used).  Prints one JSON line."""
    L = C.CDLL(path)
    L.fsaempc_ltv_workspace_bytes.restype = C.c_longlong
    vp = C.c_void_p
    L.fsaempc_ltv_step_batch_device_aux.argtypes = [C.POINTER(_lib.LtvDesc), C.POINTER(_lib.Spline)] + [vp] * 4 + [C.POINTER(_lib.QpOpts)] + [vp] * 6 + \
        [C.POINTER(_lib.QpAux), vp, C.c_longlong, vp]
    opts = _lib.QpOpts(); L.fsaempc_qp_default_opts(C.byref(opts))
    res = []
    for model, N, _ in SHAPES:
        nx, ns = (5, 1) if model == fm.KINEMATIC else (7, 4)
        x0, xl, ul, xr = fm.instances(model, N, 0.05, tr.L, 20190, range(B))
        a = [up(v) for v in (x0, xr, xl, ul)]
        xP, yP = tr.device(torch.device("cuda:0"))
        sp = _lib.Spline(tr.M, tr.dl, vp(xP.data_ptr()), vp(yP.data_ptr()))
        desc = _lib.LtvDesc(model, N, B, 0.05, -1)
        need = L.fsaempc_ltv_workspace_bytes(C.byref(desc))
        assert need > 0, need
        ws = torch.empty((need + 7) // 8, dtype=torch.float64, device="cuda")
        f64 = lambda *s: torch.empty(s, dtype=torch.float64, device="cuda")
        o = [f64(B, 2 * N), f64(B, nx * N), f64(B, ns), f64(B)]
        fl, it = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
        aux = _lib.QpAux(None, None, None, None)
        st = vp(torch.cuda.current_stream().cuda_stream)
        P = lambda t: vp(t.data_ptr())

        def step():
            rc = L.fsaempc_ltv_step_batch_device_aux(C.byref(desc), C.byref(sp), *[P(t) for t in a], C.byref(opts), *[P(t) for t in o], P(fl), P(it),
                                                     C.byref(aux), P(ws), C.c_longlong(ws.numel() * 8), st)
            assert rc == 0, rc
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        L.fsaempc_qp_set_timing(1)
        rows = []
        for _ in range(steps):
            step()
            ph = [C.c_double(0) for _ in range(4)]
            assert L.fsaempc_ltv_get_timing(*[C.byref(p) for p in ph]) == 0
            rows.append([p.value for p in ph])
        L.fsaempc_qp_set_timing(0)
        s = summary(rows)
        s.update(model=name(model), N=N, iter_mean=float(it.double().mean().item()), nonzero_exitflags=int((fl != 0).sum().item()))
        res.append(s)
    print(json.dumps(res))


if child_lib is not None:
    unblocked_with(child_lib)
    sys.exit(0)


def parent_run():
    cmd = [sys.executable, os.path.abspath(__file__), "--unblocked-with", parent_lib, out_path, str(B), str(steps), str(warmup)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def clocks():
    """What the device reports about its clocks and load (read-only query)."""
    try:
        return subprocess.run(["rocm-smi", "--showclocks", "--showuse", "--json"], capture_output=True, text=True, timeout=30).stdout.strip()[:2000]
    except Exception as e:   # noqa: BLE001 -- the note is optional
        return "unavailable: %r" % (e,)


L = fm.lib()


def phases():
    ph = [C.c_double(0) for _ in range(4)]
    assert L.fsaempc_ltv_get_timing(*[C.byref(p) for p in ph]) == 0
    return [p.value for p in ph]


res = {"what": "fused LTV-MPC step with and without move blocking, HIP events on the launch stream: median of %d steps after %d warm-up "
               "steps per variant, variants interleaved; ms" % (steps, warmup), "batch": B, "device": torch.cuda.get_device_name(0),
       "clocks_before": clocks(), "shapes": []}
parent = [parent_run()] if parent_lib else []
for model, N, lens in SHAPES:
    ns = 1 if model == fm.KINEMATIC else 4
    x0, xl, ul, xr = fm.instances(model, N, 0.05, tr.L, 20190, range(B))
    a = [up(v) for v in (x0, xr, xl, ul)]
    mpc = {"unblocked": fm.LtvBatch(model, N, 0.05, tr, B), "blocked": fm.LtvBatch(model, N, 0.05, tr, B, blocking=lens)}
    info, rows = {}, {k: [] for k in mpc}
    for k in mpc:
        for _ in range(warmup):
            o = mpc[k].step(*a, want_aux=True)
        torch.cuda.synchronize()
        f = o["exitflag"].cpu().numpy()
        info[k] = {"nV": mpc[k].nV, "nC": mpc[k].nC, "layout": fm.qp_layout(mpc[k].nV, mpc[k].nC, ns if k == "blocked" else None),
                   "iter_mean": float(o["iter"].double().mean().item()), "nonzero_exitflags": int((f != 0).sum()),
                   "exitflags": {str(v): int(c) for v, c in zip(*np.unique(f, return_counts=True))},
                   "vertex_share": float((o["polished"] > 0).double().mean().item())}
    L.fsaempc_qp_set_timing(1)
    for _ in range(steps):
        for k in mpc:
            mpc[k].step(*a)
            rows[k].append(phases())
    L.fsaempc_qp_set_timing(0)
    shape = {"model": name(model), "N": N, "blocks": lens, "variants": {k: {**summary(rows[k]), **info[k]} for k in mpc}}
    shape["blocked_vs_unblocked_step"] = shape["variants"]["blocked"]["step_ms"] / shape["variants"]["unblocked"]["step_ms"]
    res["shapes"].append(shape)
if parent_lib:
    parent.append(parent_run())
for i, shape in enumerate(res["shapes"]):
    if parent_lib:
        shape["parent_unblocked"] = [p[i] for p in parent]
        ref = min(p[i]["step_ms"] for p in parent)
    else:
        ref = shape["variants"]["unblocked"]["step_ms"]
    shape["reference_step_ms"] = ref
    shape["blocked_faster_than_parent"] = bool(shape["variants"]["blocked"]["step_ms"] < ref)

# closed loop: 256 cars x 50 steps from the Monte-Carlo starts of BASELINE configs[3], blocked next to unblocked
res["closed_loop"] = []
tr2 = fm.Track.load("fss2019")
for model, N, lens in ((fm.KINEMATIC, 40, [1] * 8 + [2] * 8 + [4] * 4), (fm.DYNAMIC, 40, [1] * 8 + [2] * 8 + [4] * 4)):
    entry = {"model": name(model), "N": N, "blocks": lens, "cars": 256, "steps": 50}
    for k, blk in (("unblocked", None), ("blocked", lens)):
        cart0, s_init = fm.monte_carlo_carts(tr2, 256, 20190)
        cl = fm.ClosedLoop(model, N, 0.05, tr2, cart0, blocking=blk)
        cl.x_opt[:, :, 0] += torch.from_numpy(s_init).to(cl.device)[:, None]
        cl.x_opt[:, :, 3] += torch.from_numpy(cart0[:, 3]).to(cl.device)[:, None]
        flags, active, pred_cost, real_cost = [], [], [], []
        for t in range(50):
            out = cl.step()
            act = cl.finished == 0
            flags.append(out["exitflag"].clone()); active.append(act); pred_cost.append(out["fval"].clone())
            real_cost.append(250.0 * cl.x0[:, 1] ** 2 + 2000.0 * cl.x0[:, 2] ** 2)   # the stage weights on n and mu (ltvmpc_*.m:32) at the car's own state
        torch.cuda.synchronize()
        fl, ac = torch.stack(flags).cpu().numpy(), torch.stack(active).cpu().numpy()
        pc, rc = torch.stack(pred_cost).cpu().numpy(), torch.stack(real_cost).cpu().numpy()
        ok = (fl == 0) & ac
        entry[k] = {"active_car_steps": int(ac.sum()), "abnormal_exits": int(((fl != 0) & ac).sum()),
                    "exitflags": {str(v): int(c) for v, c in zip(*np.unique(fl[ac], return_counts=True))},
                    "mean_predicted_cost_of_solved_steps": float(pc[ok].mean()) if ok.any() else None,
                    "median_predicted_cost_of_solved_steps": float(np.median(pc[ok])) if ok.any() else None,
                    "mean_realised_n_mu_cost": float(rc[ac].mean()) if ac.any() else None,
                    "cars_lost": int((cl.finished == 2).sum().item())}
    res["closed_loop"].append(entry)
res["clocks_after"] = clocks()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps({"shapes": [{"model": s["model"], "N": s["N"], "blocked_ms": s["variants"]["blocked"]["step_ms"],
                              "unblocked_ms": s["variants"]["unblocked"]["step_ms"], "reference_ms": s["reference_step_ms"],
                              "faster": s["blocked_faster_than_parent"]} for s in res["shapes"]]}))
