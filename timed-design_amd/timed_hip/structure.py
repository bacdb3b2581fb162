"""Structure properties of PDB files, batched on the GPU: packing density (atomic contact number, Weiss 2007) per atom and per
residue — the reference's ``tag_packing_density`` / ``_extract_packdensity_from_polypeptide`` (design_utils/analyse_utils.py:44-86,
:149-201) through th_packing_density (csrc/packdensity.hip) — and the B-factor column.

The ARITHMETIC is pinned to the reference's own functions, bit for bit (tests/golden/packdensity_golden.npz is their output).

    *** STRUCTURE RULE: PARITY UNPINNED AGAINST AMPAL ***  Which atoms of a file are neighbours and which residues are reported is
    decided in the reference by ampal's object model (``ampal.load_pdb``), and ampal is neither in the reference tree nor installed
    where this project is built — the same standing as timed_hip/voxeliser.py.  The rule implemented here is this project's own:

    * the first model of the file (``pdbio.read_pdb(path)[0]``); of alternate locations the first one seen per atom name;
    * NEIGHBOURS are all non-hydrogen atoms of ATOM and HETATM records, waters and ligands included (``include_hetero=False``
      keeps ATOM records only).  Hydrogen: element column ``H`` (any case); where the column is absent, the first letter of the
      atom name;
    * REPORTED residues are the non-hetero residues of the first chain — the chain of the first ATOM residue —, which is what the
      reference's ``assembly[0]`` iterates; ``all_chains=True`` reports the non-hetero residues of every chain;
    * atoms keep file order (the per-residue value depends on it).

Atom filters, under the reference's names (which atoms of a residue enter its value; hydrogens never do):
    ``"all"``       every non-hydrogen atom
    ``"backbone"``  N, CA, C, O
    ``"ca"``        the reference tests ``atom.res_label in "CA"`` — a SUBSTRING test on the string "CA", so it selects the atoms
                    named ``C`` and ``CA`` (and a nameless or ``A`` atom).  Reproduced as it is: published numbers were made with it
    ``"calpha"``    CA alone (an addition of this project)
The per-residue value is the reference's running half-average over the selected atoms in file order, not their mean (see
include/timed_hip.h, th_packing_density).

Rotamer labels (``tag_rotamers``; th_tag_rotamers, csrc/rotamers.hip): the chi angles of every residue and its class among the 338
categories of ``design_utils.utils.get_rotamer_codec`` — what the reference's ``tag_pdb_with_rot`` / ``extract_rotamer_encoding``
(design_utils/analyse_utils.py:901-1036) get from ampal's ``tag_sidechain_dihedrals``.

    *** ROTAMER RULE: PARITY UNPINNED AGAINST AMPAL ***  The same standing as the structure rule above.  This project's reading of
    ampal 1.5's ``classify_angle_as_rotamer`` / ``tag_sidechain_dihedrals``, written out in include/timed_hip.h (th_tag_rotamers):

    * the first model; the non-hetero residues of every chain, chains in file order (``all_chains=False``: the first chain);
    * chi k is the dihedral of atoms k .. k + 3 of the path N, CA, CB + the residue's tail (``rotamer_table``), IUPAC sign, float64;
      the first atom of a residue that carries a name is the one used (pdbio keeps the first alternate location);
    * bin 1: 0 <= chi < 120; bin 3: -120 <= chi < 0; bin 2: everything else; the first angle varies slowest in the class index;
    * unlabelled (class -1, ``None``): a residue that is not one of the 20, lacks a path atom or has a non-finite angle;
    * ALA and GLY carry their single class ``ALA_0`` / ``GLY_0`` — the only label the codec has for them; ``ala_gly_class=False``
      leaves them unlabelled, which is what a tagger that tags nothing on a residue without dihedrals would give.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib, batching, pdbio
from ._lib import ptr

ATOM_FILTERS = ("all", "ca", "backbone", "calpha")
_BACKBONE = ("N", "CA", "C", "O")
BATCH_BYTES = batching.BATCH_BYTES  # host bytes of atom arrays handed to one th_packing_density call
_ATOM_BYTES = 3 * 8 + 4 + 1 + 4     # xyz, group, selected, density
TAG_NO_ALA_GLY = 1                  # th_tag_rotamers flag bit 0: ALA and GLY stay unlabelled


def atom_selected(name: str, atom_filter: str) -> bool:
    """Does a (non-hydrogen) atom of this name enter its residue's value under ``atom_filter``?"""
    if atom_filter == "all":
        return True
    if atom_filter == "backbone":
        return name in _BACKBONE
    if atom_filter == "ca":
        return name in "CA"            # the reference's substring test: "C", "CA", "A", ""
    if atom_filter == "calpha":
        return name == "CA"
    raise ValueError(f"Atom Filter function {atom_filter} not in {ATOM_FILTERS}")


def is_hydrogen(name: str, element: str) -> bool:
    el = element.strip().upper()
    if not el or not el[0].isalpha():          # no element column and a name like "1HB": pdbio fell back to the name's first character
        el = name.lstrip("0123456789 ").upper()[:1]
    return el == "H"


@dataclass
class Layout:
    """One structure as th_packing_density takes it."""
    xyz: np.ndarray                    # [n, 3] float64, neighbours in file order
    group: np.ndarray                  # [n] int32: index into ``residues`` or -1
    selected: np.ndarray               # [n] uint8
    residues: List[pdbio.Residue]      # reported residues
    atom_names: List[Tuple[int, str]]  # per atom: (index into the model's residues, atom name)


def first_model(structure) -> pdbio.Model:
    if isinstance(structure, pdbio.Model):
        return structure
    models = pdbio.read_pdb(structure)
    if not models:
        return pdbio.Model(1, [])
    return models[0]


def reported_residues(model: pdbio.Model, all_chains: bool = False) -> List[pdbio.Residue]:
    polymer = [r for r in model.residues if not r.hetero]
    if all_chains or not polymer:
        return polymer
    return [r for r in polymer if r.chain == polymer[0].chain]


def layout(model: pdbio.Model, atom_filter: str = "ca", include_hetero: bool = True, all_chains: bool = False) -> Layout:
    """Apply the structure rule (module docstring) to one model."""
    atom_selected("CA", atom_filter)           # raises for an unknown filter
    reported = {id(r): k for k, r in enumerate(reported_residues(model, all_chains))}
    xyz, group, selected, names = [], [], [], []
    for ri, res in enumerate(model.residues):
        if res.hetero and not include_hetero:
            continue
        g = reported.get(id(res), -1)
        for name, pos in res.atoms.items():
            if is_hydrogen(name, res.elements.get(name, "")):
                continue
            xyz.append(pos)
            group.append(g)
            selected.append(1 if g >= 0 and atom_selected(name, atom_filter) else 0)
            names.append((ri, name))
    residues = [None] * len(reported)
    for r in model.residues:
        if id(r) in reported:
            residues[reported[id(r)]] = r
    return Layout(np.array(xyz, dtype=np.float64).reshape(-1, 3), np.array(group, dtype=np.int32), np.array(selected, dtype=np.uint8),
                  residues, names)


def packing_threshold(radius: float) -> float:
    """T with sqrt(s) < radius <=> s < T for every double s (th_packing_threshold; host code, no GPU needed)."""
    return float(_lib.load().th_packing_threshold(float(radius)))


def contact_numbers(xyz, offsets, radius: float = 7.0, group=None, selected=None, n_groups: int = 0, device: int = 0,
                    atoms: bool = True, timing: Optional[dict] = None):
    """One th_packing_density call.  ``xyz`` [total, 3] float64, ``offsets`` [S + 1]; ``group`` / ``selected`` [total] with
    ``n_groups`` residues (or none).  Returns (int32 [total] or None when ``atoms`` is false, float64 [n_groups]).  ``timing``: a
    dict whose ``kernel_ms`` grows by the device time of the kernel."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    if offsets.size < 1:
        raise ValueError("offsets needs at least one entry")
    total = xyz.shape[0]
    if n_groups:
        group = np.ascontiguousarray(group, dtype=np.int32).reshape(-1)
        selected = np.ascontiguousarray(selected, dtype=np.uint8).reshape(-1)
        if group.size != total or selected.size != total:
            raise ValueError(f"group and selected need {total} entries")
    density = np.empty(total, np.int32) if atoms else None
    residue = np.empty(int(n_groups), np.float64)
    ms = C.c_double(0.0)
    _lib.check(_lib.load().th_packing_density(int(device), ptr(xyz), total, ptr(offsets), offsets.size - 1, float(radius),
                                              ptr(group) if n_groups else None, ptr(selected) if n_groups else None, int(n_groups),
                                              ptr(density), ptr(residue) if n_groups else None, C.byref(ms) if timing is not None else None))
    if timing is not None:
        timing["kernel_ms"] = timing.get("kernel_ms", 0.0) + ms.value
    return density, residue


@dataclass
class StructureDensity:
    atom_density: np.ndarray           # [atoms] int32, the neighbours of the structure in file order
    residue_density: np.ndarray        # [residues] float64
    residues: List[pdbio.Residue]      # the reported residues
    layout: Layout


def cut_batches(sizes: Sequence[int], budget_bytes: int = BATCH_BYTES) -> List[Tuple[int, int]]:
    """[lo, hi) runs of consecutive structures whose atom arrays fit ``budget_bytes`` (a structure above it goes alone)."""
    return batching.cut_batches(sizes, budget_bytes, _ATOM_BYTES)


def _part_starts(part) -> Tuple[np.ndarray, np.ndarray]:
    """Where each layout of one batch starts in the batch's flat arrays: (first atom, first residue), [len(part) + 1] int64 each."""
    atom_lo, res_lo = np.zeros(len(part) + 1, np.int64), np.zeros(len(part) + 1, np.int64)
    np.cumsum([len(l.xyz) for l in part], out=atom_lo[1:])
    np.cumsum([len(l.residues) for l in part], out=res_lo[1:])
    return atom_lo, res_lo


def packing_density_layouts(layouts: Sequence[Layout], radius: float = 7.0, device: int = 0, budget_bytes: int = BATCH_BYTES,
                            stats: Optional[dict] = None) -> List[StructureDensity]:
    """The layouts through th_packing_density in as few calls as ``budget_bytes`` allows.  ``stats`` receives ``submissions`` and
    ``kernel_ms``."""
    out: List[StructureDensity] = []

    def submit(part, timing):
        offsets, res_lo = _part_starts(part)
        group = np.concatenate([np.where(l.group >= 0, l.group + res_lo[k], -1) for k, l in enumerate(part)]).astype(np.int32)
        density, residue = contact_numbers(np.concatenate([l.xyz for l in part]), offsets, radius, group,
                                           np.concatenate([l.selected for l in part]), int(res_lo[-1]), device, timing=timing)
        for k, l in enumerate(part):
            out.append(StructureDensity(density[offsets[k]:offsets[k + 1]].copy(), residue[res_lo[k]:res_lo[k + 1]].copy(), l.residues, l))
    batching.run_batches(layouts, [len(l.xyz) for l in layouts], budget_bytes, _ATOM_BYTES, submit, stats)
    return out


def packing_density(structures: Sequence[Union[pdbio.Model, str, os.PathLike]], radius: float = 7.0, atom_filter: str = "ca",
                    device: int = 0, include_hetero: bool = True, all_chains: bool = False, budget_bytes: int = BATCH_BYTES,
                    stats: Optional[dict] = None) -> List[StructureDensity]:
    """Packing density of every structure (``pdbio.Model`` objects or paths of PDB files, plain or gzipped) under the structure
    rule and the atom filters of the module docstring.  One GPU call per batch; batches are cut by ``budget_bytes`` of atom arrays,
    not per structure.  Per structure: the int32 contact number of every neighbour atom and the float64 value of every reported
    residue (-1.0 for a residue without a selected atom)."""
    layouts = [layout(first_model(s), atom_filter, include_hetero, all_chains) for s in structures]
    return packing_density_layouts(layouts, radius, device, budget_bytes, stats)


def residue_bfactors(model: pdbio.Model) -> List[List[float]]:
    """Per chain (non-hetero residues, chains in file order) the B-factor of each residue's first atom — the reference's
    ``_extract_bfactor_from_polypeptide`` (analyse_utils.py:89-109: AlphaFold2 writes one pLDDT for all atoms of a residue)."""
    chains: dict = {}
    for r in model.residues:
        if r.hetero or not r.atoms:
            continue
        first = next(iter(r.atoms))
        chains.setdefault(r.chain, []).append(float(r.bfactors.get(first, float("nan"))))
    return list(chains.values())


# ---- rotamer labels --------------------------------------------------------------------------------------------------------------
def rotamer_table() -> List[Tuple[str, int, int, Tuple[str, ...]]]:
    """th_rotamer_table for the 20 residue types in the codec's order: (three-letter code, n_chi, index of the first class, the
    n_chi + 3 path names; empty for ALA and GLY).  Host code, no GPU needed."""
    from design_utils.amino_acids import standard_amino_acids
    lib, rows = _lib.load(), []
    for t, res in enumerate(standard_amino_acids.values()):
        n_chi, base, names = C.c_int(0), C.c_int(0), C.create_string_buffer(28)
        _lib.check(lib.th_rotamer_table(t, C.byref(n_chi), C.byref(base), names))
        path = tuple(names.raw[4 * p:4 * p + 4].rstrip(b"\0").decode("ascii") for p in range(7))
        rows.append((res, n_chi.value, base.value, tuple(nm for nm in path if nm)))
    return rows


def pack_atom_names(names: Sequence[str]) -> np.ndarray:
    """atom names as th_tag_rotamers reads them: 4 ASCII bytes, left-justified, zero-padded, little-endian uint32"""
    raw = b"".join(nm.encode("ascii", "replace")[:4].ljust(4, b"\0") for nm in names)
    return np.frombuffer(raw, dtype="<u4").astype(np.uint32)


@dataclass
class RotamerLayout:
    """One structure as th_tag_rotamers takes it."""
    xyz: np.ndarray                    # [n, 3] float64, the atoms of the reported residues, residue after residue
    atom_name: np.ndarray              # [n] uint32 (pack_atom_names)
    res_offsets: np.ndarray            # [residues + 1] int64
    res_type: np.ndarray               # [residues] int8: 0..19 in the codec's order, -1 for anything else
    residues: List[pdbio.Residue]


def rotamer_layout(model: pdbio.Model, all_chains: bool = True) -> RotamerLayout:
    """Flat arrays of the non-hetero residues, chains in file order (a chain that comes back later in the file continues its
    entry).  Hydrogens stay in: they match no path name."""
    from design_utils.amino_acids import standard_amino_acids
    type_of = {res: t for t, res in enumerate(standard_amino_acids.values())}
    chains: dict = {}
    for r in reported_residues(model, all_chains):
        chains.setdefault(r.chain, []).append(r)
    residues = [r for members in chains.values() for r in members]
    offsets = np.zeros(len(residues) + 1, np.int64)
    np.cumsum([len(r.atoms) for r in residues], out=offsets[1:])
    xyz = np.array([pos for r in residues for pos in r.atoms.values()], dtype=np.float64).reshape(-1, 3)
    return RotamerLayout(xyz, pack_atom_names([nm for r in residues for nm in r.atoms]), offsets,
                         np.array([type_of.get(r.name, -1) for r in residues], dtype=np.int8), residues)


def rotamer_classes(xyz, atom_name, res_offsets, res_type, device: int = 0, ala_gly_class: bool = True, chi: bool = True,
                    timing: Optional[dict] = None):
    """One th_tag_rotamers call.  Returns (int16 [n_res], float64 [n_res, 4] or None when ``chi`` is false).  ``timing``: a dict
    that receives ``kernel_ms``."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    atom_name = np.ascontiguousarray(atom_name, dtype=np.uint32).reshape(-1)
    res_offsets = np.ascontiguousarray(res_offsets, dtype=np.int64).reshape(-1)
    res_type = np.ascontiguousarray(res_type, dtype=np.int8).reshape(-1)
    if atom_name.size != xyz.shape[0]:
        raise ValueError(f"atom_name needs {xyz.shape[0]} entries")
    if res_offsets.size != res_type.size + 1:
        raise ValueError(f"res_offsets needs {res_type.size + 1} entries")
    n_res = res_type.size
    cls = np.empty(n_res, np.int16)
    angles = np.empty((n_res, 4), np.float64) if chi else None
    ms = C.c_double(0.0)
    _lib.check(_lib.load().th_tag_rotamers(int(device), ptr(xyz), ptr(atom_name), xyz.shape[0], ptr(res_offsets), ptr(res_type), n_res,
                                           0 if ala_gly_class else TAG_NO_ALA_GLY, ptr(cls), ptr(angles),
                                           C.byref(ms) if timing is not None else None))
    if timing is not None:
        timing["kernel_ms"] = timing.get("kernel_ms", 0.0) + ms.value
    return cls, angles


@dataclass
class StructureRotamers:
    residues: List[pdbio.Residue]      # the non-hetero residues, chains in file order
    cls: np.ndarray                    # [residues] int16: index into get_rotamer_codec()[1], -1 unlabelled
    chi: np.ndarray                    # [residues, 4] float64 degrees, NaN where there is no such angle

    @property
    def rotamers(self) -> List[Optional[str]]:
        """the bins of each residue as the codec spells them: "13", "2212", "0" for ALA / GLY, None when unlabelled"""
        from design_utils.utils import get_rotamer_codec
        names = get_rotamer_codec()[1]
        return [None if c < 0 else names[c].split("_")[1] for c in self.cls.tolist()]


def tag_rotamer_layouts(layouts: Sequence[RotamerLayout], device: int = 0, ala_gly_class: bool = True, budget_bytes: int = BATCH_BYTES,
                        stats: Optional[dict] = None) -> List[StructureRotamers]:
    """The layouts through th_tag_rotamers in as few calls as ``budget_bytes`` allows (cut_batches, as packing_density_layouts).
    ``stats`` receives ``submissions`` and ``kernel_ms``."""
    out: List[StructureRotamers] = []

    def submit(part, timing):
        atom_lo, res_lo = _part_starts(part)
        offsets = np.concatenate([l.res_offsets[:-1] + atom_lo[k] for k, l in enumerate(part)] + [atom_lo[-1:]])
        cls, chi = rotamer_classes(np.concatenate([l.xyz for l in part]), np.concatenate([l.atom_name for l in part]), offsets,
                                   np.concatenate([l.res_type for l in part]), device, ala_gly_class, timing=timing)
        for k, l in enumerate(part):
            out.append(StructureRotamers(l.residues, cls[res_lo[k]:res_lo[k + 1]].copy(), chi[res_lo[k]:res_lo[k + 1]].copy()))
    batching.run_batches(layouts, [len(l.xyz) for l in layouts], budget_bytes, _ATOM_BYTES, submit, stats)
    return out


def tag_rotamers(structures: Sequence[Union[pdbio.Model, RotamerLayout, str, os.PathLike]], device: int = 0, ala_gly_class: bool = True,
                 budget_bytes: int = BATCH_BYTES, stats: Optional[dict] = None) -> List[StructureRotamers]:
    """Chi angles and rotamer classes of every structure (``pdbio.Model`` objects, ``RotamerLayout`` objects or paths of PDB files,
    plain or gzipped) under the rotamer rule of the module docstring.  One GPU call per batch; batches are cut by ``budget_bytes``
    of atom arrays, not per structure."""
    layouts = [s if isinstance(s, RotamerLayout) else rotamer_layout(first_model(s)) for s in structures]
    return tag_rotamer_layouts(layouts, device, ala_gly_class, budget_bytes, stats)


def labels_for_map(tagged: StructureRotamers, dataset_map_rows) -> Tuple[List[Optional[int]], int]:
    """The classes of one tagged structure in DATASET-MAP order: ``dataset_map_rows`` are rows of an old-format map (pdb, chain,
    residue number, label), all of this structure; each is matched on (chain, residue number as pdbio writes it, insertion code
    included).  Returns (labels, unmatched): ``None`` for a row whose residue the structure lacks or that is unlabelled, and the
    count of rows without a matching residue.  The reference pairs labels and matrix rows BY POSITION and silently misaligns when
    a structure has residues the map lacks; positional pairing stays the default wherever the reference does it — this is the
    opt-in alternative."""
    by_key = {}
    for r, c in zip(tagged.residues, tagged.cls.tolist()):
        by_key.setdefault((r.chain, r.number), c)
    labels, unmatched = [], 0
    for row in dataset_map_rows:
        key = (str(row[1]).strip(), str(row[2]).strip())
        if key not in by_key:
            unmatched += 1
            labels.append(None)
        else:
            labels.append(None if by_key[key] < 0 else int(by_key[key]))
    return labels, unmatched
