#!/usr/bin/env python
"""Generate tests/golden/sasa_golden.npz: the tables of th_sasa's rule (include/timed_hip.h) on the cases of its write-up — the heavy
polymer atoms of tests/golden/1ubq.pdb1.gz at 96 and at 960 points and with a probe of 0, 1ubq plus a rigidly moved copy as chain B
(the interface), 1ubq with a three-atom pseudo-ligand on its first three water sites, and the analytic cases (a lone atom, two equal
spheres 3 and 6 Angstrom apart, a sphere inside another, a point exactly on a neighbour's sphere and just inside it) — computed by the
NumPy restatement tests/sasa_restatement.py in float64: NOT by the kernel, and NOT by FreeSASA, NACCESS, DSSP or Biopython, which are
not available; the rule is this project's own (PARITY UNPINNED AGAINST FREESASA / NACCESS / DSSP / BIOPYTHON).

The direction vectors are th_sasa_sphere's (host code of the library, no GPU), stored in the file as ``points_96``, ``points_960`` and
``points_tie``, so that whoever reads the fixture sees the doubles it was made with.  Holds per case ``<case>_exposed`` (int32 [n]),
``<case>_mask`` (uint64 [n, ceil(P / 64)]) and ``<case>_totals`` (int64 [3]); for the 1ubq cases ``<case>_residue_area`` (float64
[4, residues]: all, polar, apolar, backbone) and ``<case>_area`` (float64 [3]: all, polar, apolar over every atom); for the dimer
``ubq_dimer_area_lost`` [152] and ``ubq_dimer_interface``; and ``cases``.  The inputs are rebuilt by sasa_restatement.cases().

The figures of the rule's write-up are asserted here before anything is written.

Usage:  python tests/golden/make_sasa_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "timed-design_amd"))
import sasa_restatement as sr  # noqa: E402
from timed_hip import sasa  # noqa: E402


def check_write_up(arrays, points):
    """the numbers of the rule's write-up, from a CPU prototype of the same rule"""
    xyz, radius, group, polar, backbone, names = sr.ubq_atoms()
    atoms = sr.read_atoms()
    waters = {(a["chain"], a["number"]) for a in atoms if a["record"] == "HETATM"}
    assert len(xyz) == 602 and len(names) == 76 and len(waters) == 58 and all(a["residue"] in sr.WATERS for a in atoms if a["record"] == "HETATM")
    for n, total in ((96, 4895.6), (192, 4862.6), (960, 4872.5)):
        one = sr.restate(xyz, radius, sr.PROBE, points[n], every_pair=True)
        area = sr.atom_areas(one["exposed"], radius, sr.PROBE, n)
        sums, totals = sr.residue_areas(area, group, polar, backbone, 76)
        print(f"1ubq at {n} points: total {totals[0]:.1f} polar {totals[1]:.1f} apolar {totals[2]:.1f}, neighbours max {one['n_near'].max()} "
              f"mean {one['n_near'].mean():.1f}, ties {one['ties']}, buried atoms {int(one['totals'][1])}")
        assert one["ties"] == 0 and abs(totals[0] - total) < 0.05, (n, totals)
        if n == 96:
            assert one["n_near"].max() == 59 and abs(one["n_near"].mean() - 37.0) < 0.05
            assert abs(totals[1] - 2760.2) < 0.05 and abs(totals[2] - 2135.4) < 0.05 and one["totals"][1] == 271
            classes = sr.burial(sums[0] / np.array([sr.MAX_ASA[nm] for nm in names]))
            assert [classes.count(k) for k in (0, 1, 2)] == [24, 35, 17], classes
            assert abs(sums[0][75] / sr.MAX_ASA["GLY"] - 1.4) < 0.05 and names[75] == "GLY"
    for name, want in sr.ANALYTIC.items():
        assert arrays[f"{name}_exposed"].tolist() == want, (name, arrays[f"{name}_exposed"].tolist())
    # coincident atoms of equal radius: what survives is what the rounding of |u_k| decides — the same for both, neither 0 nor all
    for place, radius, probe, survive in (((0.0, 0.0, 0.0), 1.7, 1.4, 76), ((1.0, 2.0, 3.0), 1.5, 1.5, 80)):
        coincident = sr.restate(np.array([place, place]), np.array([radius, radius]), probe, points[96])
        print("coincident atoms at", place, "R", radius + probe, "->", coincident["exposed"].tolist())
        assert coincident["exposed"].tolist() == [survive, survive], coincident["exposed"].tolist()
    assert arrays["ubq_dimer_interface"] > 100.0 and (arrays["ubq_dimer_area_lost"] > 0).sum() >= 10
    assert not (arrays["ubq_hetero_exposed"][:602] == arrays["ubq_exposed"]).all() and (arrays["ubq_hetero_exposed"][602:] > 0).all()


def main():
    points = {n: sasa.sphere_points(n) for n in (96, 192, 960)}
    arrays = sr.golden_arrays(points[96], points[960])
    check_write_up(arrays, points)
    np.savez_compressed(sr.GOLDEN, **arrays)
    print("wrote", sr.GOLDEN, os.path.getsize(sr.GOLDEN), "bytes")
    for name in sr.CASES:
        print(f"{name:12s} valid, buried, exposed points {arrays[name + '_totals'].tolist()}")
    print("dimer interface", float(arrays["ubq_dimer_interface"]), "residues that lose area", int((arrays["ubq_dimer_area_lost"] > 0).sum()))


if __name__ == "__main__":
    main()
