#!/usr/bin/env python3
"""Diagnostic (QP_PROBE build): cycles of pass 1 alone vs inside the solver (compare with tools/phase_profile.py), and whether fp64
VALU work runs beside the fp64 MFMAs of the same wave (overlap_probe_kernel: 16 MFMAs; 32 v_fma_f64; both interleaved)."""
import ctypes as C, os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
import fsae_mpc_amd as fm

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
tr = fm.Track.load("fsg2019")
x0, xl, ul, xr = fm.instances(fm.KINEMATIC, 40, 0.05, tr.L, 20190, range(B))
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
q = fm.LtvBatch(fm.KINEMATIC, 40, 0.05, tr, B).build_qp(up(x0), up(xr), up(xl), up(ul))
dump = torch.zeros(2 * B + 64, dtype=torch.float64, device="cuda")
fm.lib().fsaempc_debug_set_dump(C.c_void_p(dump.data_ptr()), 8)
for _ in range(2):
    out = fm.qp_solve_batch_device(*(q[k] for k in ("H", "g", "A", "lb", "ub", "lbA", "ubA")))
    torch.cuda.synchronize()
fm.lib().fsaempc_debug_set_dump(None, 0)
d = dump.cpu().numpy()
print("pass 1 alone: %.0f cycles/pass (mean over %d QPs), min %.0f max %.0f ; checksum[0] %.6e" % (d[:B].mean(), B, d[:B].min(), d[:B].max(), d[B]))
o = d[2 * B:2 * B + 4]
print("overlap probe, cycles per trip (block 0): 16 MFMA %.0f | 32 v_fma_f64 %.0f | 16 MFMA + 32 v_fma_f64 interleaved %.0f (sum of the parts %.0f) ; checksum %.6e"
      % (o[0], o[1], o[2], o[0] + o[1], o[3]))
