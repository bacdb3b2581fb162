"""Writes tests/golden/seqset_golden.npz: the inputs of the th_seqset cases and all their tables, computed by the NumPy restatement
(tests/seqset_restatement.py) from the rule in include/timed_hip.h — NOT by the kernel.  The clustering (the incremental scheme of
CD-HIT-like tools in its plainest form) is THIS PROJECT'S OWN RULE, NOT THEIR CODE: the fixture pins the rule as written.

    python tests/golden/make_seqset_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "timed-design_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import seqset_restatement as qr  # noqa: E402


def main():
    arrays = qr.golden_arrays()
    for name in ("ubq_drift", "ubq_drift_07"):
        n = len(arrays[f"{name}_codes"])
        distinct, clusters = int(arrays[f"{name}_set"][1]), int(arrays[f"{name}_set"][2])
        print(name, "distinct", distinct, "clusters", clusters, "of", n)
        assert 1 < clusters < n and distinct == 68
    np.savez_compressed(qr.GOLDEN, **arrays)
    print(qr.GOLDEN, os.path.getsize(qr.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
