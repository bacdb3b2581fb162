"""Writes tests/golden/seqalign_golden.npz: the inputs of the th_seqalign cases and, for every setting (two tables, three gap pairs,
free and charged ends), align and counts — computed by the plain restatement (tests/seqalign_restatement.py) from the rule in
include/timed_hip.h, NOT by the kernel.  PARITY UNPINNED AGAINST PYMOL: the fixture pins this project's own rule as written, not
cmd.align.  The five cases of the rule's table must come out at the figures the rule was first run at, or nothing is written.

    python tests/golden/make_seqalign_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "timed-design_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import seqalign_restatement as ar  # noqa: E402


def main():
    arrays = ar.golden_arrays()
    for name, (free, charged, aligned) in ar.TABLE.items():
        got = [arrays[f"{name}_blosum_free_counts"].tolist(), arrays[f"{name}_blosum_global_counts"].tolist()]
        print(name, got)
        assert (got[0][2], got[1][2], got[0][3], got[1][3]) == (free, charged, aligned, aligned), name
    np.savez_compressed(ar.GOLDEN, **arrays)
    print(ar.GOLDEN, os.path.getsize(ar.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
