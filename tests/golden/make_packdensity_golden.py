#!/usr/bin/env python
"""Generate tests/golden/packdensity_golden.npz by RUNNING the reference's own packing-density functions — build container only.

The reference's design_utils/analyse_utils.py imports once its heavyweight module-level imports are stubbed (the stubs of
make_sampler_golden.py); ``tag_packing_density`` and ``_extract_packdensity_from_polypeptide`` are plain NumPy over duck-typed
objects, so they run on hand-made ``Assembly`` / chain / residue / atom objects (``get_atoms()``, ``.element``, ``.array``,
``.res_label``, ``.tags``; the class has to be NAMED Assembly).  Nothing of the reference travels: the fixture holds what it
computed, the sha256 of the seeded synthetic coordinates (tests/packdensity_restatement.py rebuilds them) and the coordinates of
tests/golden/1ubq.pdb1.gz as timed_hip.pdbio reads them.

Per case: ``<case>_density_r<radius>`` (int32 per non-hydrogen atom, tag_packing_density at every radius of RADII) and
``<case>_res_<filter>_r<radius>`` (float64 per residue of the first chain, _extract_packdensity_from_polypeptide for its three
filters).  The latter function calls tag_packing_density with its default radius (7); for the other radii that default is
rebound for the call — the code that runs is still the reference's.

Usage:  python tests/golden/make_packdensity_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import packdensity_restatement as pr  # noqa: E402
from make_sampler_golden import stub_modules  # noqa: E402


class Atom:
    def __init__(self, res_label, element, array):
        self.res_label, self.element, self.array = res_label, element, np.asarray(array, dtype=np.float64)
        self.tags = {}


class Residue(list):
    pass


class Chain(list):
    pass


class Assembly(list):
    def get_atoms(self):
        for chain in self:
            for res in chain:
                yield from res


def assembly_of(chains):
    return Assembly(Chain(Residue(Atom(nm, el, pos) for nm, el, pos in res["atoms"]) for res in chain) for chain in chains)


def ubq_chains():
    """1ubq under the structure rule of timed_hip/structure.py, written out independently: first model, first chain's non-hetero
    residues reported (chain 0), everything else a neighbour (chain 1)"""
    sys.path.insert(0, os.path.join(ROOT, "timed-design_amd"))
    from timed_hip import pdbio
    model = pdbio.read_pdb(os.path.join(HERE, "1ubq.pdb1.gz"))[0]
    first = next(r.chain for r in model.residues if not r.hetero)
    chains = [[], []]
    for r in model.residues:
        atoms = [(nm, "H" if r.elements[nm].upper() == "H" else r.elements[nm], pos) for nm, pos in r.atoms.items()]
        chains[0 if (not r.hetero and r.chain == first) else 1].append(dict(name=r.name, number=r.number, hetero=r.hetero, atoms=atoms))
    return chains


def run_reference(ref, chains, name, out):
    for radius in pr.RADII:
        asm = assembly_of(chains)
        with np.errstate(invalid="ignore", over="ignore"):
            ref.tag_packing_density(asm, radius=radius)
        heavy = [a for a in asm.get_atoms() if a.element != "H"]
        out[f"{name}_density_r{radius}"] = np.array([a.tags["packing density"] for a in heavy], dtype=np.int32)
        original = ref.tag_packing_density
        defaults = original.__defaults__
        for atom_filter in pr.FILTERS:
            asm = assembly_of(chains)
            original.__defaults__ = (radius,)              # the default radius _extract_packdensity_from_polypeptide tags with
            try:
                with np.errstate(invalid="ignore", over="ignore"):
                    values = ref._extract_packdensity_from_polypeptide(asm, atom_filter)
            finally:
                original.__defaults__ = defaults
            out[f"{name}_res_{atom_filter}_r{radius}"] = np.array(values, dtype=np.float64)


def main():
    stub_modules()
    sys.path.insert(0, REF)
    from design_utils import analyse_utils as ref

    out = {"numpy_version": np.array(np.__version__)}
    for name in pr.GOLDEN_CASES:
        chains = pr.golden_structure(name)
        if not chains[0]:
            chains[0] = []
        out[f"{name}_sha256"] = np.array(pr.coords_sha256(chains))
        run_reference(ref, chains, name, out)
    chains = ubq_chains()
    out["ubq_xyz"] = pr.flatten(chains, "all")[0]
    run_reference(ref, chains, "ubq", out)
    path = os.path.join(HERE, "packdensity_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(out), "arrays;", len(out["ubq_xyz"]), "atoms of 1ubq")
    for name in list(pr.GOLDEN_CASES) + ["ubq"]:
        d = out[f"{name}_density_r7.0"]
        print(name, len(d), "atoms; density r7 min/max", (d.min(), d.max()) if len(d) else None, "; residues",
              len(out[f"{name}_res_ca_r7.0"]), "; -1 residues (ca)", int((out[f"{name}_res_ca_r7.0"] == -1).sum()))


if __name__ == "__main__":
    main()
