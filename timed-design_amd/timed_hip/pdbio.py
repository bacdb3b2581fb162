"""Minimal PDB reader for the voxeliser: ATOM/HETATM records of fixed-column PDB files, plain or
gzipped (the reference ships tests/testing_files/1ubq.pdb1.gz and passes ``is_pdb_gzipped`` to aposteriori, ui.py:81).
Only what voxelisation needs: coordinates, atom / residue names, chain, residue number (+ insertion code), element,
model number.  Alternate locations: the first one seen for an atom name within a residue wins (blank or 'A').
The temperature factor (columns 61-66; AlphaFold2 writes pLDDT there) is kept per atom for timed_hip.structure.
``write_pdb`` writes one model back as fixed-column records (timed_hip.sidechains: the native backbone with built side chains).
``find_structures`` / ``stem_of``: which files of a directory the command-line programs take for structures, and their labels.
"""
from __future__ import annotations

import gzip
from dataclasses import dataclass, field
from pathlib import Path
from typing import Dict, List, Tuple

import numpy as np

PDB_SUFFIXES = (".pdb", ".pdb1", ".ent")


def is_pdb_name(name: str) -> bool:
    name = name.lower()
    if name.endswith(".gz"):
        name = name[:-3]
    return name.endswith(PDB_SUFFIXES)


def find_structures(entries):
    """[(label, path)]: a file as it is (labelled by its name), a directory searched recursively for *.pdb, *.pdb1, *.ent, each
    optionally .gz (labelled by the path below the directory), in sorted order"""
    found = []
    for entry in entries:
        entry = Path(entry)
        if entry.is_dir():
            found += [(str(p.relative_to(entry)), p) for p in sorted(entry.rglob("*")) if p.is_file() and is_pdb_name(p.name)]
        elif entry.is_file():
            found.append((entry.name, entry))
        else:
            raise FileNotFoundError(f"No structure file or directory at {entry}")
    return found


def stem_of(label: str) -> str:
    name = Path(label).name
    if name.lower().endswith(".gz"):
        name = name[:-3]
    return name.rsplit(".", 1)[0]


@dataclass
class Residue:
    chain: str
    number: str            # residue number + insertion code as written ("12", "12A")
    name: str              # three-letter code
    atoms: Dict[str, np.ndarray] = field(default_factory=dict)   # atom name -> xyz (float64)
    elements: Dict[str, str] = field(default_factory=dict)
    hetero: bool = False
    bfactors: Dict[str, float] = field(default_factory=dict)     # atom name -> B-factor (NaN when the column is absent or unparsable)


@dataclass
class Model:
    number: int
    residues: List[Residue]


def _open(path):
    path = str(path)
    if path.endswith(".gz"):
        return gzip.open(path, "rt", encoding="ascii", errors="replace")
    return open(path, "r", encoding="ascii", errors="replace")


def read_pdb(path) -> List[Model]:
    """All models of the file (a file without MODEL records is one model, number 1)."""
    models: List[Model] = []
    residues: List[Residue] = []
    index: Dict[Tuple[str, str, str], Residue] = {}
    number = 1

    def close_model():
        nonlocal residues, index
        if residues:
            models.append(Model(number, residues))
        residues, index = [], {}

    with _open(path) as f:
        for line in f:
            rec = line[:6]
            if rec == "MODEL ":
                close_model()
                try:
                    number = int(line[10:14])
                except ValueError:
                    number = len(models) + 1
            elif rec == "ENDMDL":
                close_model()
                number += 1
            elif rec in ("ATOM  ", "HETATM") and len(line) >= 54:
                name = line[12:16].strip()
                resname = line[17:20].strip()
                chain = line[21].strip() or "A"
                resnum = (line[22:26].strip() + line[26].strip())
                try:
                    xyz = np.array([float(line[30:38]), float(line[38:46]), float(line[46:54])])
                except ValueError:
                    continue
                key = (chain, resnum, resname)
                res = index.get(key)
                if res is None:
                    res = index[key] = Residue(chain, resnum, resname, hetero=rec == "HETATM")
                    residues.append(res)
                if name in res.atoms:            # another alternate location of an atom we already have
                    continue
                res.atoms[name] = xyz
                el = line[76:78].strip() if len(line) >= 78 else ""
                res.elements[name] = el or name[:1]
                try:
                    res.bfactors[name] = float(line[60:66])
                except ValueError:                   # a short line, blanks, or not a number
                    res.bfactors[name] = float("nan")
    close_model()
    return models


def element_of(name: str) -> str:
    """the element of a protein heavy atom or hydrogen from its name: the first letter behind any leading digits ("CA" is carbon)"""
    letters = name.lstrip("0123456789 ")
    return letters[:1].upper()


def _name_column(name: str, element: str) -> str:
    """columns 13-16: a four-character name fills them; a shorter one starts in column 14 unless its element has two letters"""
    if len(name) >= 4:
        return name[:4]
    if len(element) == 2 and name.upper().startswith(element.upper()):
        return name.ljust(4)
    return (" " + name).ljust(4)


def write_pdb(path, model: Model) -> int:
    """Write one model as fixed-column ATOM / HETATM records, residue after residue in the model's order: serial numbers from 1,
    occupancy 1.00, the B-factor of ``Residue.bfactors`` (0.00 where absent or NaN), the element of ``Residue.elements`` or else
    from the name (``element_of``), a TER record where the chain changes and after the last residue, then END.  Coordinates are
    written with three decimals.  A path ending in .gz is gzipped.  Returns the number of atoms written; ``read_pdb`` of the file
    gives the same residues, names and the coordinates rounded to three decimals."""
    lines, serial = [], 0
    residues = model.residues

    def number_of(res):
        number = res.number.strip()
        icode = number[-1] if number and number[-1].isalpha() else " "
        return (number[:-1] if icode != " " else number)[-4:].rjust(4), icode
    for r, res in enumerate(residues):
        number, icode = number_of(res)
        for name, pos in res.atoms.items():
            serial += 1
            element = (res.elements.get(name) or element_of(name)).strip().upper()[:2]
            if not element.isalpha():
                element = element_of(name)
            b = res.bfactors.get(name, 0.0)
            b = 0.0 if b != b else b
            lines.append("%-6s%5d %4s %3s %1s%4s%1s   %8.3f%8.3f%8.3f%6.2f%6.2f          %2s\n" % (
                "HETATM" if res.hetero else "ATOM", serial % 100000, _name_column(name, element), res.name[:3].rjust(3), res.chain[:1] or "A",
                number, icode, pos[0], pos[1], pos[2], 1.0, b, element.rjust(2)))
        if r + 1 == len(residues) or residues[r + 1].chain != res.chain:
            serial += 1
            lines.append("TER   %5d      %3s %1s%4s%1s\n" % (serial % 100000, res.name[:3].rjust(3), res.chain[:1] or "A", number, icode))
    lines.append("END\n")
    path = str(path)
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "wt", encoding="ascii") as f:
        f.writelines(lines)
    return serial - sum(1 for line in lines if line.startswith("TER"))
