"""fsaempc_selftest_initial_point (the device self test of the solve kernel's start-up pass: A~x and A~'w of the initial multipliers from
one pass against a pass of its own for each) on the host side: declared, exported, and without a device it says so with a negative
value, never a made-up pass."""
import os
import re

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_initial_point_selftest_is_declared_and_exported():
    import fsae_mpc_amd as fm
    hdr = open(os.path.join(ROOT, "include", "fsaempc.h")).read()
    assert re.search(r"\bint\s+fsaempc_selftest_initial_point\s*\(\s*void\s*\)\s*;", hdr)
    assert "fsaempc_selftest_initial_point" in fm._lib.EXPORTS and hasattr(fm.lib(), "fsaempc_selftest_initial_point")


def test_initial_point_selftest_needs_a_device():
    import torch
    import fsae_mpc_amd as fm
    rc = fm.lib().fsaempc_selftest_initial_point()
    if torch.cuda.is_available():
        assert rc == 0, fm.lib().fsaempc_last_error()
    else:
        assert rc < 0 and b"no HIP device" in fm.lib().fsaempc_last_error()
