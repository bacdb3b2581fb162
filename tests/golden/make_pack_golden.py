#!/usr/bin/env python
"""Generate tests/golden/pack_golden.npz: 1ubq packed under the rule of th_pack_sidechains (include/timed_hip.h) by the NumPy
restatement tests/pack_restatement.py — NOT by the kernel, and not by SCWRL4, which is not available: the rule is this project's
own (PARITY UNPINNED AGAINST SCWRL4).

Four cases (pack_restatement.fixture_cases): ``native`` — the native sequence, no prior, the default ladder; ``prior`` — the same
under a seeded Dirichlet matrix through packer.prior_costs; ``predicted`` — a seeded synthetic sequence on the same backbone;
``single_level`` — ladder (2.5), weight 1.  Per case ``<case>_cls``, ``_cost_initial``, ``_cost_final``, ``_energy`` (initial,
final), ``_search`` (sweeps, moves, converged, status), ``_margin``, ``_types`` and, with a prior, ``_prior``; for the two cases
on the native sequence also ``_chi1`` (chi1 bins right, residues with a chi angle), ``_rmsd`` and ``_pairs`` (side-chain RMSD to
the deposited atoms and clashing pairs under 2.5 Angstrom of the packed classes built at their bin centres).  ``sha256`` of the
input as timed_hip.pdbio reads it.

It also prints the table of the README: what the first class of every residue, the native classes at their bin centres and the
search under three ladders reach on 1ubq.

Usage:  python tests/golden/make_pack_golden.py [--check]      (--check: write nothing, print the table only)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "timed-design_amd"))
import pack_restatement as pr  # noqa: E402
import rotamer_restatement as rr  # noqa: E402
import sidechain_restatement as sr  # noqa: E402


def measures(residues, cls, natives, native_cls):
    """(side-chain RMSD to the deposited atoms, clashing pairs under 2.5 Angstrom, chi1 bins right, residues with a chi angle) of
    the classes built at their bin centres"""
    build = [(res, bb, sr.class_centres(int(c))[1] if c >= 0 else np.full(4, np.nan)) if c >= 0 else ("GLY", bb, np.full(4, np.nan))
             for (res, bb), c in zip(residues, cls)]
    xyz, n_built = sr.restate_build(build)
    n_matched, sum_sq = sr.restate_match(build, xyz, n_built, natives)
    _, pairs, _ = sr.restate_clashes(build, xyz, np.zeros(len(build), np.int32), np.array([0, len(build)]))
    right, total = pr.chi1_right(residues, cls, native_cls)
    return sr.overall_rmsd(n_matched, sum_sq), int(pairs[0]), right, total


def compute():
    residues, native_cls, sha = pr.ubq_structure()
    _, natives, _ = sr.ubq_inputs()
    out = dict(sha256=np.array(sha))
    for name, (res, chain, prior, kw) in pr.fixture_cases().items():
        got = pr.restate_pack(res, chain, prior=prior, **kw)
        assert got["margin"] > pr.MARGIN_BOUND, (name, got["margin"])
        out[name + "_cls"] = got["cls"]
        out[name + "_cost_initial"] = got["cost_initial"]
        out[name + "_cost_final"] = got["cost_final"]
        out[name + "_energy"] = np.array([got["energy_initial"], got["energy_final"]], np.int64)
        out[name + "_search"] = np.array([got["n_sweeps"], got["n_moves"], got["converged"], got["status"]], np.int32)
        out[name + "_margin"] = np.array(got["margin"])
        out[name + "_types"] = np.array([sr.type_index(r[0]) for r in res], np.int8)
        if prior is not None:
            out[name + "_prior"] = np.asarray(prior, np.int32)
        line = f"{name}: energy {got['energy_initial']} -> {got['energy_final']} in {got['n_sweeps']} sweeps, {got['n_moves']} moves, converged {got['converged']}, margin {got['margin']:.2e}"
        if name in ("native", "single_level"):
            rmsd, pairs, right, total = measures(res, got["cls"], natives, native_cls)
            out[name + "_chi1"] = np.array([right, total], np.int32)
            out[name + "_rmsd"] = np.array(rmsd)
            out[name + "_pairs"] = np.array(pairs, np.int64)
            line += f"; RMSD {rmsd:.3f}, {pairs} clashing pairs, chi1 {right} of {total}"
        print(line)
    return out


def table():
    residues, native_cls, _ = pr.ubq_structure()
    _, natives, _ = sr.ubq_inputs()
    first = np.array([rr.CLASS_BASE[res] if pr.n_candidates(res) else -1 for res, _ in residues], np.int16)
    rows = [("first class everywhere", first, ""), ("native classes at bin centres", native_cls, "")]
    for ladder in ((2.5,), pr.LADDER, pr.LADDER + (4.0,)):
        got = pr.restate_pack(residues, ladder=ladder)
        rows.append((f"search, ladder {ladder}", got["cls"], f"{got['n_sweeps']} sweeps, {got['n_moves']} moves, margin {got['margin']:.1e}"))
    print("| 1ubq | side-chain RMSD | clashing pairs < 2.5 | chi1 bin right | search |")
    for name, cls, note in rows:
        rmsd, pairs, right, total = measures(residues, cls, natives, native_cls)
        print(f"| {name} | {rmsd:.3f} | {pairs} | {right} of {total} | {note} |")


def main():
    out = compute()
    table()
    if "--check" not in sys.argv:
        np.savez_compressed(pr.GOLDEN, **out)
        print("wrote", pr.GOLDEN, os.path.getsize(pr.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
