#!/usr/bin/env python
"""Generate tests/golden/secstruct_golden.npz: the tables of th_secondary_structure's rule (include/timed_hip.h) on the cases of its
write-up — the backbone of tests/golden/1ubq.pdb1.gz (76 residues), the same without residues 30 .. 35 (counted from 0), four ideal
backbones built by NeRF (alpha, 3-10, pi, beta), the alpha-helix with two chain ids after residue 9 and the alpha-helix with the O of
residue 7 missing — computed by the NumPy restatement tests/secstruct_restatement.py in float64: NOT by the kernel, and NOT by mkdssp,
PyMOL's dss or STRIDE, which are not available; the rule is this project's own (PARITY UNPINNED AGAINST DSSP).

Holds per case ``<case>_cls`` (uint8 [L]), ``<case>_residue`` (int32 [L, 6]), ``<case>_totals`` (int64 [10]: n_valid, n_hbonds, the
eight class counts) and ``<case>_bits`` (uint64 [L * ceil(L / 64)]: row = acceptor, bit = donor); and ``cases``.  The inputs are
rebuilt by secstruct_restatement.cases().

Usage:  python tests/golden/make_secstruct_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import secstruct_restatement as ss  # noqa: E402


def main():
    arrays = ss.golden_arrays()
    np.savez_compressed(ss.GOLDEN, **arrays)
    print("wrote", ss.GOLDEN, os.path.getsize(ss.GOLDEN), "bytes")
    for name in ss.CASES:
        print(f"{name:10s} n_valid, n_hbonds, counts {arrays[name + '_totals'].tolist()}  {ss.as_string(arrays[name + '_cls'])}")


if __name__ == "__main__":
    main()
