#!/usr/bin/env python
"""Generate tests/golden/lddt_atoms_golden.npz: the integer tables of th_lddt_atoms' rule (include/timed_hip.h) at the default radius
(15) and thresholds (0.5, 1, 2, 4) on the cases of tests/lddt_atoms_restatement.py — the 601 heavy atoms of tests/golden/1ubq.pdb1.gz
against themselves, with every symmetric name pair exchanged, with 0.3 Angstrom of noise (and exchanged), with ten side chains
absent from the model (as NaN and as an infinity), with non-finite reference coordinates and with five residues renamed; hand-made
pairs whose decisions sit exactly on a tie; synthetic chains of 257, 300, 256 and 1 atoms around the kernels' tile of 256 —
computed by the NumPy restatement in float64: NOT by the kernel, and NOT by OpenStructure, which is not available; the rule is this
project's own (PARITY UNPINNED AGAINST OPENSTRUCTURE).

Holds per case its inputs ``<case>_ref``, ``_mob`` (float64 [n, 3]), ``_residue``, ``_partner`` (int32 [n]), the resolved tables
``<case>_atom`` (int32 [n, 5]), ``_swapped`` (uint8 [n]), ``_pair`` (int64 [8]: n_ref, n_missing, N, C[0..3], n_swapped_residues) and
the tables under TH_LDDT_NO_SYMMETRY ``<case>_named_atom`` ...; ``cases``; and ``sha256`` of the inputs.

Every case but the hand-made ties must keep every float decision further than 1e-9 Angstrom from its boundary (the margin
tests/test_gpu_lddt.py asks of the CA cases) and must have no symmetric residue with swap_R == keep_R; float64 and long double must
give the same integers.  The maker asserts all three.  ``missing_symmetric`` is a tie case of its own kind: symmetric residues whose
partnered atoms the model lacks have swap_R == keep_R == 0, which no rounding can move; its float margin is asserted like the others'.

Usage:  python tests/golden/make_lddt_atoms_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "timed-design_amd"))
import lddt_atoms_restatement as ar  # noqa: E402


def main():
    cases = ar.build_cases()
    for name, case in cases.items():
        inputs = [case[key] for key in ar.INPUTS]
        res, exact = ar.restate(*inputs), ar.restate(*inputs, dtype=np.longdouble)
        named = ar.restate(*inputs, symmetry=False)
        print(f"{name:20s} atoms {len(case['ref']):4d} pair {res['pair'].tolist()} lddt {ar.score(res['pair']):.4f} as named "
              f"{ar.score(named['pair']):.4f} edge {res['edge']:.3e} margin {res['margin']}")
        if name in ar.TIES:
            continue
        assert res["edge"] > ar.EDGE and named["edge"] > ar.EDGE, (name, res["edge"], named["edge"])
        if name in ar.MARGIN_TIES:
            assert res["margin"] == 0 and all(res["keep"][r] == 0 for r in res["keep"] if res["swap"][r] == res["keep"][r]), name     # 0 = 0 only
        else:
            assert res["margin"] > 0, (name, res["keep"], res["swap"])
        for table in ar.TABLES:
            assert res[table].tobytes() == exact[table].tobytes(), (name, table)
    arrays = ar.golden_arrays(cases)
    np.savez_compressed(ar.GOLDEN, **arrays)
    print("wrote", ar.GOLDEN, os.path.getsize(ar.GOLDEN), "bytes; inputs", str(arrays["sha256"])[:16])


def part(rows, mask):
    total = rows[mask].astype(np.int64).sum(axis=0)
    return float(total[1:].sum()) / (4.0 * float(total[0]))


def packing_table():
    """The rows of the README's packing table (tests/golden/make_pack_golden.py) re-scored: the classes built at their bin centres
    by the side-chain restatement on the native backbone, against the deposited 1ubq, as named and with the names resolved."""
    import make_pack_golden as mp
    import pack_restatement as pr
    import rotamer_restatement as rr
    import sidechain_restatement as sr
    from timed_hip import pdbio
    native = ar.ubq()
    residues, native_cls, _ = pr.ubq_structure()
    deposited = [r for r in native.residues if not r.hetero]
    assert [r.name for r in deposited] == [res for res, _ in residues]
    first = np.array([rr.CLASS_BASE[res] if pr.n_candidates(res) else -1 for res, _ in residues], np.int16)
    rows = [("first class everywhere", first), ("native classes at bin centres", native_cls)]
    for ladder in ((2.5,), pr.LADDER, pr.LADDER + (4.0,)):
        rows.append((f"search, ladder {ladder}", pr.restate_pack(residues, ladder=ladder)["cls"]))
    _, natives, _ = sr.ubq_inputs()
    print("| 1ubq | side-chain RMSD | lddt_sidechain as named | lddt_sidechain | lddt | residues swapped |")
    for name, cls in rows:
        built = []
        for old, (res, backbone), c in zip(deposited, residues, cls):
            new = pdbio.Residue(old.chain, old.number, old.name, {a: old.atoms[a] for a in ar.BACKBONE if a in old.atoms})
            atoms = sr.build_residue(res, backbone, sr.class_centres(int(c))[1]) if c >= 0 else None
            new.atoms.update(atoms or {})
            new.elements = {a: a[:1] for a in new.atoms}
            built.append(new)
        ref, mob, residue, partner, backbone, _ = ar.lists_of_models(native, pdbio.Model(1, built))
        resolved, named = ar.restate(ref, mob, residue, partner), ar.restate(ref, mob, residue, partner, symmetry=False)
        rmsd = mp.measures(residues, cls, natives, native_cls)[0]
        print(f"| {name} | {rmsd:.3f} | {part(named['atom'], ~backbone):.4f} | {part(resolved['atom'], ~backbone):.4f} | "
              f"{ar.score(resolved['pair']):.4f} | {int(resolved['pair'][7])} | missing {int(resolved['pair'][1])}")


if __name__ == "__main__":
    if "--packing-table" in sys.argv:
        packing_table()
    else:
        main()
