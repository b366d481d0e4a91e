"""fsaempc_selftest_lane_reduce (the device self test of the solve kernel's cross-lane reductions) on the host side: declared,
exported, and -- like fsaempc_selftest_mfma -- it reports the missing device with a negative value, never a made-up pass."""
import os
import re

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_lane_reduce_selftest_is_declared_and_exported():
    import fsae_mpc_amd as fm
    hdr = open(os.path.join(ROOT, "include", "fsaempc.h")).read()
    assert re.search(r"\bint\s+fsaempc_selftest_lane_reduce\s*\(\s*void\s*\)\s*;", hdr)
    assert "fsaempc_selftest_lane_reduce" in fm._lib.EXPORTS and hasattr(fm.lib(), "fsaempc_selftest_lane_reduce")


def test_lane_reduce_selftest_needs_a_device():
    import torch
    import fsae_mpc_amd as fm
    rc = fm.lib().fsaempc_selftest_lane_reduce()
    if torch.cuda.is_available():
        assert rc == 0, fm.lib().fsaempc_last_error()
    else:
        assert rc < 0 and b"no HIP device" in fm.lib().fsaempc_last_error()
