"""fsaempc_selftest_diag_factor (the device self test of the register Cholesky's diagonal tiles: the newer forms of diag_factor against
the former one) on the host side: declared, exported, and without a device it says so with a negative value, never a made-up pass."""
import os
import re

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_diag_factor_selftest_is_declared_and_exported():
    import fsae_mpc_amd as fm
    hdr = open(os.path.join(ROOT, "include", "fsaempc.h")).read()
    assert re.search(r"\bint\s+fsaempc_selftest_diag_factor\s*\(\s*void\s*\)\s*;", hdr)
    assert "fsaempc_selftest_diag_factor" in fm._lib.EXPORTS and hasattr(fm.lib(), "fsaempc_selftest_diag_factor")


def test_diag_factor_selftest_needs_a_device():
    import torch
    import fsae_mpc_amd as fm
    rc = fm.lib().fsaempc_selftest_diag_factor()
    if torch.cuda.is_available():
        assert rc == 0, fm.lib().fsaempc_last_error()
    else:
        assert rc < 0 and b"no HIP device" in fm.lib().fsaempc_last_error()
