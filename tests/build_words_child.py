#!/usr/bin/env python3
"""Child process of tests/test_build_repro_gpu.py::test_builds_reproduce_across_processes: runs every build of
exact_cases.repro_cases() once (the twelve instantiations of ltv_build_kernel, N = 20, B = 16, seed 31) in a process of its own
and stores the raw 64-bit words of every output tensor.  usage: build_words_child.py <out.npz>"""
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import exact_cases as ec
    builds = ec.ReproBuilds()
    res = {}
    for case in ec.repro_cases():
        for k, w in builds.run(case).items():
            res["%s/%s" % (ec.repro_id(case), k)] = w
    np.savez(sys.argv[1], **res)
    print("ok", len(res), "tensors")


if __name__ == "__main__":
    main()
