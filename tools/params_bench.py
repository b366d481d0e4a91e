#!/usr/bin/env python3
"""Cost of the runtime parameter block: build phase and whole fused step, by the library's HIP events
(fsaempc_ltv_get_timing), at B = 4096 for kinematic N = 40 and dynamic N = 60, three ways in the same run -- the entry with the
constants compiled in, the parameterised entry with one shared default block, the parameterised entry with one
param_draws(spread = 0.1) block per instance -- with the exit-flag tallies of the three.  Warm-up steps first, then the median of
`steps` (>= 20) timed steps per variant, the variants interleaved round-robin so that clock drift hits all three alike.
usage: params_bench.py [out.json] [B=4096] [steps=30] [warmup=5]"""
import ctypes as C, json, os, subprocess, sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
import fsae_mpc_amd as fm

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "params", "params_bench_B4096.json")
B = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
steps = max(20, int(sys.argv[3])) if len(sys.argv) > 3 else 30
warmup = int(sys.argv[4]) if len(sys.argv) > 4 else 5
L = fm.lib()
tr = fm.Track.load("fsg2019")
up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()


def clocks():
    """What the device reports about its clocks and load before the run (read-only query)."""
    try:
        return subprocess.run(["rocm-smi", "--showclocks", "--showuse", "--json"], capture_output=True, text=True, timeout=30).stdout.strip()[:2000]
    except Exception as e:   # noqa: BLE001 -- the note is optional
        return "unavailable: %r" % (e,)


def phases():
    ph = [C.c_double(0) for _ in range(4)]
    assert L.fsaempc_ltv_get_timing(*[C.byref(p) for p in ph]) == 0
    return [p.value for p in ph]


res = {"what": "fused LTV-MPC step, HIP events on the launch stream: median of %d steps after %d warm-up steps per variant, variants "
               "interleaved; ms" % (steps, warmup), "batch": B, "device": torch.cuda.get_device_name(0), "clocks_before": clocks(), "shapes": []}
for model, N in ((fm.KINEMATIC, 40), (fm.DYNAMIC, 60)):
    x0, xl, ul, xr = fm.instances(model, N, 0.05, tr.L, 20190, range(B))
    a = [up(v) for v in (x0, xr, xl, ul)]
    variants = {"fixed": None, "shared_default": fm.default_params(model), "per_instance_draws": fm.param_draws(model, np.arange(B), 20190, 0.1)}
    mpc = {k: fm.LtvBatch(model, N, 0.05, tr, B, params=p) for k, p in variants.items()}
    rows = {k: [] for k in variants}
    flags = {}
    for k in variants:
        for _ in range(warmup):
            o = mpc[k].step(*a)
        torch.cuda.synchronize()
        f = o["exitflag"].cpu().numpy()
        flags[k] = {str(v): int(c) for v, c in zip(*np.unique(f, return_counts=True))}
    L.fsaempc_qp_set_timing(1)
    for _ in range(steps):
        for k in variants:
            mpc[k].step(*a)
            rows[k].append(phases())
    L.fsaempc_qp_set_timing(0)
    shape = {"model": "dynamic" if model == fm.DYNAMIC else "kinematic", "N": N, "variants": {}}
    for k in variants:
        r = np.array(rows[k])
        shape["variants"][k] = {"build_ms_median": float(np.median(r[:, 0])), "build_ms_min": float(r[:, 0].min()), "build_ms_max": float(r[:, 0].max()),
                                "step_ms_median": float(np.median(r.sum(1))), "prep_ms_median": float(np.median(r[:, 1])),
                                "solve_ms_median": float(np.median(r[:, 2])), "post_ms_median": float(np.median(r[:, 3])), "exitflags": flags[k]}
    fx = shape["variants"]["fixed"]["build_ms_median"]
    for k in ("shared_default", "per_instance_draws"):
        shape["variants"][k]["build_vs_fixed"] = shape["variants"][k]["build_ms_median"] / fx
    res["shapes"].append(shape)
res["clocks_after"] = clocks()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps({"shapes": [{"model": s["model"], "N": s["N"], **{k: (v["build_ms_median"], v["step_ms_median"], v["exitflags"]) for k, v in s["variants"].items()}}
                             for s in res["shapes"]]}))
