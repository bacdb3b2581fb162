#!/usr/bin/env python
"""Generate tests/golden/tmscore_golden.npz: the outputs of th_tmscore's rule (include/timed_hip.h) on the five cases of the
superposition fixture — the 76 CA atoms of tests/golden/1ubq.pdb1.gz against a rigid copy, sigma = 0.5 noise, a re-oriented tail
("hinge"), the mirror image and a pair with non-finite positions — computed by the NumPy restatement tests/tmscore_restatement.py in
float64: NOT by the kernel, and NOT by Zhang & Skolnick's TMscore program, which is not available; the rule is this project's own
(PARITY UNPINNED AGAINST THE TM-score PROGRAM).

Holds per case ``<case>_tm`` and ``<case>_d0`` (float64), ``<case>_counts`` (int64 [4]: n_valid, L, n_seeds, n_fits),
``<case>_winner`` (int64 [2]: the seed and the round of the best score), ``<case>_edge_gap`` (float64 [2]: the nearest any d_i came
to a cut, the smallest relative eigenvalue gap of a fit) and ``<case>_tm_global_fit`` (the same sum under the one least-squares fit
over all valid positions); ``cases``; and ``sha256`` of the input coordinates, which are rebuilt from the seed by
superpose_restatement.ubq_cases — the same inputs as superpose_golden.npz.  20 rounds, L = 76.

Usage:  python tests/golden/make_tmscore_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import superpose_restatement as sr  # noqa: E402
import tmscore_restatement as tr  # noqa: E402


def main():
    arrays = tr.golden_arrays()
    np.savez_compressed(tr.GOLDEN, **arrays)
    print("wrote", tr.GOLDEN, os.path.getsize(tr.GOLDEN), "bytes; inputs", str(arrays["sha256"])[:16])
    for name in sr.CASES:
        print(f"{name:8s} tm {float(arrays[f'{name}_tm']):.5f} (global fit {float(arrays[f'{name}_tm_global_fit']):.5f}) d0 {float(arrays[f'{name}_d0']):.5f} "
              f"counts {arrays[f'{name}_counts'].tolist()} edge / gap {arrays[f'{name}_edge_gap'].tolist()}")


if __name__ == "__main__":
    main()
