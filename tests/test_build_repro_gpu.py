"""Reproducibility of the twelve instantiations of ltv_build_kernel, word for word: a build is a deterministic program, so its
outputs may depend neither on what its output buffers held, nor on what an earlier kernel left in LDS and registers, nor on the
process it runs in.  N = 20, B = 16, seed 31: the shape at which the exact kinematic RK4 build with compiled-in constants was
recorded as differing from one process to the next (profiles/build_unify/README.md)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import exact_cases as ec

pytestmark = pytest.mark.gpu

CASES = ec.repro_cases()


@pytest.fixture(scope="module")
def builds():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return ec.ReproBuilds()


def _differing(a, b):
    return {k: int((a[k] != b[k]).sum()) for k in a if not np.array_equal(a[k], b[k])}


@pytest.mark.parametrize("case", CASES, ids=ec.repro_id)
def test_build_reproduces_in_one_process(builds, case):
    """Three runs: into outputs pre-filled with zero bytes, into outputs pre-filled with 0xFF bytes (a word the kernel leaves
    unwritten, or reads before it writes it, shows), and after an unrelated fused dynamic N = 40 step."""
    zero = builds.run(case, 0)
    ones = builds.run(case, 0xFF)
    builds.unrelated_step()
    after = builds.run(case, 0)
    assert not _differing(zero, ones), ("zeros against 0xFF", _differing(zero, ones))
    assert not _differing(zero, after), ("before against after another kernel", _differing(zero, after))


@pytest.fixture(scope="module")
def two_processes(tmp_path_factory):
    """The child twice, one after the other, each a fresh process."""
    d = tmp_path_factory.mktemp("build_words")
    out = []
    for i in range(2):
        path = str(d / ("run%d.npz" % i))
        r = subprocess.run([sys.executable, os.path.join(ec.ROOT, "tests", "build_words_child.py"), path], cwd=ec.ROOT, timeout=120,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, (i, r.stdout[-2000:], r.stderr[-4000:])
        out.append(dict(np.load(path)))
    return out


@pytest.mark.parametrize("case", CASES, ids=ec.repro_id)
def test_builds_reproduce_across_processes(two_processes, case):
    a, b = ({k.split("/")[1]: v for k, v in run.items() if k.startswith(ec.repro_id(case) + "/")} for run in two_processes)
    assert len(a) == 10 and sorted(a) == sorted(b)
    assert not _differing(a, b), _differing(a, b)
