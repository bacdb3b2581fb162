#!/usr/bin/env python
"""Generate tests/golden/rotamer_tags_golden.npz: the rotamer classes and chi angles of tests/golden/1ubq.pdb1.gz under the rule of
th_tag_rotamers (include/timed_hip.h), computed by the NumPy restatement tests/rotamer_restatement.py in float64 — NOT by the
kernel, and not by ampal, which is not available: the rule is this project's own (PARITY UNPINNED AGAINST AMPAL).

Holds ``cls`` (int16 [76]), ``chi`` (float64 [76, 4], NaN where there is no such angle) and ``sha256`` of the residue names, atom
names and coordinates as timed_hip.pdbio reads them.

Usage:  python tests/golden/make_rotamer_tags_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "timed-design_amd"))
import rotamer_restatement as rr  # noqa: E402
from timed_hip import pdbio  # noqa: E402


def main():
    residues = rr.residues_of_model(pdbio.read_pdb(rr.UBQ)[0])
    cls, chi = rr.restate(residues)
    np.savez_compressed(rr.GOLDEN, cls=cls, chi=chi, sha256=np.array(rr.coords_sha256(residues)), numpy_version=np.array(np.__version__))
    print("wrote", rr.GOLDEN, os.path.getsize(rr.GOLDEN), "bytes;", len(cls), "residues,", int((cls >= 0).sum()), "labelled,",
          int(np.isfinite(chi).sum()), "chi angles,", len(set(cls.tolist())), "distinct classes; nearest bin edge",
          rr.edge_distance(chi), "degrees")
    print("first twenty classes", cls[:20].tolist())


if __name__ == "__main__":
    main()
