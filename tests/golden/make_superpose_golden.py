#!/usr/bin/env python
"""Generate tests/golden/superpose_golden.npz: the outputs of th_superpose's rule (include/timed_hip.h) on five cases derived from the
76 CA atoms of tests/golden/1ubq.pdb1.gz — a rigid copy, sigma = 0.5 noise, a re-oriented tail ("hinge"), the mirror image and a pair
with non-finite positions — computed by the NumPy restatement tests/superpose_restatement.py in float64: NOT by the kernel, and NOT
by PyMOL, which is not available; the rule is this project's own (PARITY UNPINNED AGAINST PYMOL).

Holds per case ``<case>_dist`` (float64 [76]), ``<case>_kept`` (uint8 [76]), ``<case>_rmsd`` (float64 [3]: kept, all, fit_all),
``<case>_counts`` (int32 [7]) and ``<case>_transform`` (float64 [12]); ``cases``; and ``sha256`` of the input coordinates, which are
rebuilt from the seed by superpose_restatement.ubq_cases.  The rigid case runs with cycles = 0, the others with 5 (see CASE_CYCLES).

Usage:  python tests/golden/make_superpose_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import superpose_restatement as sr  # noqa: E402


def main():
    arrays = sr.golden_arrays()
    np.savez_compressed(sr.GOLDEN, **arrays)
    print("wrote", sr.GOLDEN, os.path.getsize(sr.GOLDEN), "bytes; inputs", str(arrays["sha256"])[:16])
    for name in sr.CASES:
        print(f"{name:8s} rmsd kept / all / fit_all", arrays[f"{name}_rmsd"].tolist(), "counts", arrays[f"{name}_counts"].tolist())


if __name__ == "__main__":
    main()
