#!/usr/bin/env python
"""Generate tests/golden/sidechain_golden.npz: the side chains of tests/golden/1ubq.pdb1.gz rebuilt from N, CA, C, the residue types
and the NATIVE chi angles under the rule of th_build_sidechains (include/timed_hip.h), computed by the NumPy restatement
tests/sidechain_restatement.py in float64 — NOT by the kernel, and not by SCWRL4, which is not available: the table is this
project's own (PARITY UNPINNED AGAINST SCWRL4).

First the table check by data: for every row of the tree that 1ubq covers, the table's bond length, bond angle and dihedral offset
beside the mean and spread of the deposited atoms; then the rebuild and its RMSD to the deposited side chains, which must stay
<= 0.40 Angstrom (the per-type means of 1ubq itself give 0.331); then ring closure and planarity.

Holds ``xyz`` (float64 [76, 10, 3], NaN-padded), ``n_built``, ``n_matched`` (int32 [76]), ``sum_sq`` (float64 [76]), ``clashes``
(int32 [76]) and ``pairs`` (int64 [1]) at 2.5 Angstrom with N, CA, C, O as backbone, ``rmsd`` (the table-check figure) and
``sha256`` of the residue names, atom names and coordinates as timed_hip.pdbio reads them.

Usage:  python tests/golden/make_sidechain_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "timed-design_amd"))
import rotamer_restatement as rr  # noqa: E402
import sidechain_restatement as sr  # noqa: E402

RMSD_BOUND = 0.40


def wrap(x):
    return (x + 180.0) % 360.0 - 180.0


def angle(a, b, c):
    u, v = a - b, c - b
    return np.degrees(np.arccos(u @ v / np.linalg.norm(u) / np.linalg.norm(v)))


def table_against_data(residues, natives):
    seen = {}
    for (res, _, chi), (_, atoms) in zip(residues, natives):
        first = {}
        for name, pos in atoms:
            first.setdefault(name, np.asarray(pos, np.float64))
        for name, (a, b, c), k, length, theta, off in sr.TREE.get(res, []):
            if not all(n in first for n in (name, a, b, c)):
                continue
            base = chi[k] if k >= 0 else 0.0
            key = ("*" if name == "CB" else res, name)
            seen.setdefault(key, [(length, theta, off)]).append(
                (np.linalg.norm(first[name] - first[c]), angle(first[b], first[c], first[name]),
                 wrap(rr.dihedral(first[a], first[b], first[c], first[name]) - base - off)))
    print("row          n   length: table, 1ubq mean +- sd    angle: table, mean +- sd    offset: table, mean deviation (worst)")
    for (res, name), rows in sorted(seen.items()):
        (length, theta, off), v = rows[0], np.array(rows[1:])
        print(f"{res:3s} {name:4s} {len(v):4d}   {length:.3f}  {v[:, 0].mean():.3f} +- {v[:, 0].std():.3f}      {theta:6.1f}  {v[:, 1].mean():6.1f} +- "
              f"{v[:, 1].std():4.1f}     {off:7.1f}  {v[:, 2].mean():+6.1f} ({np.abs(v[:, 2]).max():.1f})")


def main():
    residues, natives, sha = sr.ubq_inputs()
    table_against_data(residues, natives)
    xyz, n_built = sr.restate_build(residues)
    n_matched, sum_sq = sr.restate_match(residues, xyz, n_built, natives)
    rmsd = sr.overall_rmsd(n_matched, sum_sq)
    per = np.sqrt(sum_sq[n_matched > 0] / n_matched[n_matched > 0])
    worst = int(np.argmax(np.where(n_matched > 0, sum_sq / np.maximum(n_matched, 1), 0)))
    print(f"1ubq rebuilt from native chi: {int((n_built > 0).sum())} residues, {int(n_matched.sum())} atoms matched, RMSD {rmsd:.4f} Angstrom "
          f"(bound {RMSD_BOUND}), median per residue {np.median(per):.3f}, worst {residues[worst][0]} {worst + 1} {per.max():.3f}")
    assert rmsd <= RMSD_BOUND, "a row of the table is wrong: fix the row, not the bound"
    closures, planar = sr.closure_and_planarity()
    for res, a, b, stated, got in closures:
        print(f"closure {res} {a}-{b}: stated {stated:.3f}, built {got:.4f}")
        assert abs(got - stated) <= 0.05
    print("planarity (Angstrom off the ring plane):", {k: float(f"{v:.2e}") for k, v in planar.items()})
    assert max(planar.values()) <= 0.02
    offsets = np.array([0, len(residues)])
    clashes, pairs, margin = sr.restate_clashes(residues, xyz, np.zeros(len(residues), np.int32), offsets)
    print(f"clashes at {sr.CLASH_DISTANCE} Angstrom: {int(pairs[0])} pairs, {int((clashes > 0).sum())} residues; nearest distance to the threshold {margin:.2e}")
    np.savez_compressed(sr.GOLDEN, xyz=xyz, n_built=n_built, n_matched=n_matched, sum_sq=sum_sq, clashes=clashes, pairs=pairs,
                        rmsd=np.array(rmsd), sha256=np.array(sha), numpy_version=np.array(np.__version__))
    print("wrote", sr.GOLDEN, os.path.getsize(sr.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
