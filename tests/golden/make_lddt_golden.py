#!/usr/bin/env python
"""Generate tests/golden/lddt_golden.npz: the integer tables of th_lddt's rule (include/timed_hip.h) at the default radius (15) and
thresholds (0.5, 1, 2, 4) on the five cases derived from the 76 CA atoms of tests/golden/1ubq.pdb1.gz that the superposition fixture
uses — a rigid copy, sigma = 0.5 noise, a re-oriented tail ("hinge"), the mirror image and a pair with non-finite positions —
computed by the NumPy restatement tests/lddt_restatement.py in float64: NOT by the kernel, and NOT by OpenStructure or AlphaFold's
lddt.py, which are not available; the rule is this project's own (PARITY UNPINNED AGAINST OPENSTRUCTURE).

Holds per case ``<case>_residue`` (int32 [76, 5]: n_i, c_i[0..3]) and ``<case>_pair`` (int64 [6]: n_valid, N, C[0..3]); ``cases``;
and ``sha256`` of the input coordinates, which are rebuilt from the seed by superpose_restatement.ubq_cases.

Usage:  python tests/golden/make_lddt_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import lddt_restatement as lr  # noqa: E402


def main():
    arrays = lr.golden_arrays()
    np.savez_compressed(lr.GOLDEN, **arrays)
    print("wrote", lr.GOLDEN, os.path.getsize(lr.GOLDEN), "bytes; inputs", str(arrays["sha256"])[:16])
    for name in lr.CASES:
        pair = arrays[f"{name}_pair"]
        print(f"{name:8s} n_valid {pair[0]} N {pair[1]} C {pair[2:].tolist()} lddt {lr.score(pair):.4f}")


if __name__ == "__main__":
    main()
