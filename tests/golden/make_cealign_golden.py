#!/usr/bin/env python
"""Generate tests/golden/cealign_golden.npz: the outputs of th_cealign's rule (include/timed_hip.h) on seven cases — the 76 CA atoms of
tests/golden/1ubq.pdb1.gz against a rigid copy, sigma = 0.5 noise, a re-oriented tail ("hinge") and the mirror image (the inputs of
superpose_golden.npz), against a model that lacks residues 30 .. 35 ("deletion") and one with a 10-residue loop after position 40
("insertion"), and an ideal 40-residue helix against an ideal strand — computed by the NumPy restatement tests/cealign_restatement.py
in float64: NOT by the kernel, and NOT by PyMOL, which is not available; the rule is this project's own (PARITY UNPINNED AGAINST PYMOL).

Holds per case ``<case>_counts`` (int64 [6]: mA, mB, n_starts, n_afps, n_aligned, n_candidates), ``<case>_align`` (int32 [nA]: the
model position aligned to each reference position, -1 if none) and ``<case>_rmsd`` (float64 [2]: the RMSD over the aligned positions,
the winning path's score); ``cases``; and ``sha256`` of the input coordinates, which are rebuilt from the seed by
cealign_restatement.ubq_cases.  Window 8, d0 3.0, d1 4.0, gap_max 30, 20 candidates.

Usage:  python tests/golden/make_cealign_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import cealign_restatement as cr  # noqa: E402


def main():
    arrays = cr.golden_arrays()
    np.savez_compressed(cr.GOLDEN, **arrays)
    print("wrote", cr.GOLDEN, os.path.getsize(cr.GOLDEN), "bytes; inputs", str(arrays["sha256"])[:16])
    for name in cr.CASES:
        print(f"{name:12s} counts {arrays[f'{name}_counts'].tolist()} rmsd, score {arrays[f'{name}_rmsd'].tolist()}")


if __name__ == "__main__":
    main()
