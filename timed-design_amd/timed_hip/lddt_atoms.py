"""All-atom lDDT with symmetric side chains, batched on the GPU: the local Distance Difference Test (Mariani et al. 2013) of every
(reference, model) pair over the heavy atoms of the paired residues, per atom, per residue and per pair, through th_lddt_atoms
(csrc/lddt_atoms.hip).  This is the lDDT that CASP, CAMEO and OpenStructure quote, and the superposition-free measure of side-chain
placement: a PHE ring turned by 180 degrees is the same molecule, so the names of chemically equivalent atoms are resolved per
residue before anything is counted.  ``timed_hip.lddt`` is the CA-only form; the side-chain RMSD of ``timed_hip.sidechains`` pairs
atoms by name with no symmetry correction.

    *** PARITY UNPINNED AGAINST OPENSTRUCTURE ***  OpenStructure is not available where this project is built.  The rule is this
    project's reading of the published definition, written out in include/timed_hip.h: float64, no stereochemistry checks, no
    sequence-separation filter, strict inequalities on both tests.  It is not OpenStructure's code.

    * residues are read and paired exactly as ``timed_hip.superpose`` does (``pair_by="position"`` or ``"number"``, or what
      ``cealign.prepare_aligned`` returned); no sequence alignment is made;
    * the REFERENCE's atoms define the list (``atom_lists``): its heavy atoms in file order — hydrogens and deuterium dropped by
      element, ``OXT`` dropped, no hetero residues.  A model atom is found by name in the paired residue, or is MISSING: it stays in
      every count of included pairs and is preserved at no threshold, so a missing atom costs score;
    * where the paired residues' names differ only N, CA, C, O of that reference residue enter: its side chain is neither scored nor
      counted as missing, and the residue is counted in ``n_mismatched_residues``;
    * an ordered pair of atoms (i, j) is included when both have finite reference coordinates, lie in different residues and are
      closer than ``radius`` (15 Angstrom) in the reference; it is preserved at a threshold t (0.5, 1, 2, 4 Angstrom) when the model's
      distance differs from the reference's by less than t; ``lddt`` is the mean over the thresholds of the preserved fraction of ALL
      ordered pairs — pair-weighted;
    * SYMMETRY: ``design_utils.amino_acids.SYMMETRIC_ATOMS`` (WRITTEN FROM MEMORY, NOT FETCHED) names the atom pairs of ASP, GLU,
      PHE, TYR, ARG, LEU and VAL that may exchange names; a partner is set only when both names are present in the reference
      residue.  A residue is swapped — all its pairs together — iff that preserves more of its distances to atoms WITHOUT a partner;
      a tie keeps the names.  ``symmetry=False`` scores the model as named;
    * out of scope: stereochemistry checks, sequence-separation filters, ligands, sequence alignment, hydrogens, NMR ensembles.
"""
from __future__ import annotations

import ctypes as C
import csv
from dataclasses import dataclass
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _lib, pdbio, structure
from ._lib import ptr
from .lddt import RADIUS, THRESHOLDS, fractions
from .superpose import AtomLayout, prepare, score_pairs
from .textio import float_repr as _fmt

TH_LDDT_NO_SYMMETRY = 1                    # include/timed_hip.h
BACKBONE = ("N", "CA", "C", "O")
_ATOM_BYTES = 2 * 3 * 8 + 4 + 4 + 5 * 4 + 1  # both coordinate lists, residue, partner, the row of counts, the swapped byte
MODEL_COLUMNS = ["label", "reference", "model", "n_atoms", "n_missing", "n_mismatched_residues", "n_included", "lddt", "preserved_0.5",
                 "preserved_1", "preserved_2", "preserved_4", "lddt_backbone", "lddt_sidechain", "n_swapped_residues", "error"]
RESIDUE_COLUMNS = ["label", "chain", "number", "residue", "model_residue", "n_atoms", "n_missing", "n_included", "lddt", "swapped"]


class LddtAtomTables(NamedTuple):
    """What one th_lddt_atoms call returns."""
    atom: np.ndarray                   # [total, 5] int32: n_i, c_i[0..3]; zeros at an atom that is not reference-valid
    swapped: np.ndarray                # [total] uint8: 1 where the model coordinates used were the partner's
    pair: np.ndarray                   # [pairs, 8] int64: n_ref, n_missing, N, C[0..3], n_swapped_residues


def lddt_atoms_arrays(ref_xyz, mob_xyz, residue, partner, offsets, radius: float = RADIUS, thresholds: Sequence[float] = THRESHOLDS,
                      symmetry: bool = True, device: int = 0, timing: Optional[dict] = None) -> LddtAtomTables:
    """One th_lddt_atoms call.  ``ref_xyz`` / ``mob_xyz`` [total, 3] float64, ``residue`` / ``partner`` [total] int32 (local to their
    pair), ``offsets`` [pairs + 1].  ``timing``: a dict whose ``kernel_ms`` grows by the device time of all kernels and whose
    ``resolve_ms`` by that of the symmetry resolution alone."""
    ref_xyz = np.ascontiguousarray(ref_xyz, dtype=np.float64).reshape(-1, 3)
    mob_xyz = np.ascontiguousarray(mob_xyz, dtype=np.float64).reshape(-1, 3)
    residue = np.ascontiguousarray(residue, dtype=np.int32).reshape(-1)
    partner = np.ascontiguousarray(partner, dtype=np.int32).reshape(-1)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    limits = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
    if offsets.size < 1:
        raise ValueError("offsets needs at least one entry")
    total, n_pairs = ref_xyz.shape[0], offsets.size - 1
    if mob_xyz.shape[0] != total or residue.size != total or partner.size != total:
        raise ValueError(f"ref_xyz has {total} atoms, mob_xyz {mob_xyz.shape[0]}, residue {residue.size}, partner {partner.size}")
    if limits.size != 4:
        raise ValueError(f"four thresholds are needed, got {limits.size}")
    atom = np.empty((total, 5), np.int32)
    swapped = np.empty(total, np.uint8)
    pair = np.empty((n_pairs, 8), np.int64)
    ms = (C.c_double * 2)(0.0, 0.0)
    _lib.check(_lib.load().th_lddt_atoms(int(device), ptr(ref_xyz), ptr(mob_xyz), ptr(residue), ptr(partner), total, ptr(offsets), n_pairs,
                                         float(radius), ptr(limits), 0 if symmetry else TH_LDDT_NO_SYMMETRY, ptr(atom), ptr(swapped), ptr(pair),
                                         C.cast(ms, C.POINTER(C.c_double)) if timing is not None else None))
    if timing is not None:
        timing["kernel_ms"] = timing.get("kernel_ms", 0.0) + ms[0] + ms[1]
        timing["resolve_ms"] = timing.get("resolve_ms", 0.0) + ms[0]
    return LddtAtomTables(atom, swapped, pair)


class AtomLists(NamedTuple):
    """The flat arrays of one pair of paired residue lists."""
    ref_xyz: np.ndarray                # [n, 3] float64
    mob_xyz: np.ndarray                # [n, 3] float64, NaN at a missing atom
    residue: np.ndarray                # [n] int32: index into ``residue_at``, from 0 in steps of 0 or 1
    partner: np.ndarray                # [n] int32: index of the atom that may exchange names with this one, or -1
    backbone: np.ndarray               # [n] bool: N, CA, C, O
    names: List[str]                   # [n] atom names
    residue_at: np.ndarray             # [residues with atoms] int64: position in the paired lists of residue index r
    n_mismatched_residues: int


def _heavy(res: pdbio.Residue, name: str) -> bool:
    element = res.elements.get(name, "").strip().upper()
    if not element or not element[0].isalpha():
        element = pdbio.element_of(name)
    return element not in ("H", "D")


def atom_lists(reference_residues: Sequence[pdbio.Residue], model_residues: Sequence[pdbio.Residue]) -> AtomLists:
    """The arrays of th_lddt_atoms for one pair: ``reference_residues[k]`` is paired with ``model_residues[k]``.  The rules are
    those of the module docstring: the reference's heavy atoms in file order, no OXT, no hetero residues; a model atom by name or
    NaN; N, CA, C, O alone where the residue names differ; partners from SYMMETRIC_ATOMS when both names are present."""
    from design_utils.amino_acids import SYMMETRIC_ATOMS
    if len(reference_residues) != len(model_residues):
        raise ValueError(f"{len(reference_residues)} reference residues are paired with {len(model_residues)} model residues")
    ref_xyz, mob_xyz, residue, partner, backbone, names, residue_at = [], [], [], [], [], [], []
    mismatched = 0
    missing = np.full(3, np.nan)
    for k, (ours, theirs) in enumerate(zip(reference_residues, model_residues)):
        if ours.hetero:
            continue
        same = ours.name == theirs.name
        mismatched += 0 if same else 1
        taken = [name for name in ours.atoms if name != "OXT" and _heavy(ours, name) and (same or name in BACKBONE)]
        if not taken:
            continue
        first = len(names)
        for name in taken:
            ref_xyz.append(ours.atoms[name])
            mob_xyz.append(theirs.atoms.get(name, missing))
            residue.append(len(residue_at))
            partner.append(-1)
            backbone.append(name in BACKBONE)
            names.append(name)
        if same:
            for a, b in SYMMETRIC_ATOMS.get(ours.name, ()):
                if a in taken and b in taken:
                    partner[first + taken.index(a)], partner[first + taken.index(b)] = taken.index(b) + first, taken.index(a) + first
        residue_at.append(k)
    return AtomLists(np.array(ref_xyz, dtype=np.float64).reshape(-1, 3), np.array(mob_xyz, dtype=np.float64).reshape(-1, 3),
                     np.array(residue, dtype=np.int32), np.array(partner, dtype=np.int32), np.array(backbone, dtype=bool), names,
                     np.array(residue_at, dtype=np.int64), mismatched)


@dataclass
class LddtAtomsResult:
    error: Optional[str]               # why the pair was not scored (every figure below is then NaN / 0 / empty)
    n_atoms: int                       # reference-valid atoms
    n_missing: int                     # of those, atoms the model lacks
    n_mismatched_residues: int         # paired residues whose names differ: backbone only
    n_included: int                    # N: ordered included pairs
    preserved: Tuple[float, float, float, float]       # C[k] / N at the four thresholds
    lddt: float                        # sum_k C[k] / (4 N): pair-weighted
    lddt_backbone: float               # the same sums over the rows of N, CA, C, O atoms
    lddt_sidechain: float              # ... and over the rows of the other atoms
    n_swapped_residues: int
    n_i: np.ndarray                    # [paired residues] int64: included pairs of the residue's atoms
    lddt_i: np.ndarray                 # [paired residues] float64, NaN where n_i = 0
    swapped: np.ndarray                # [paired residues] uint8
    atoms_i: np.ndarray                # [paired residues] int32: atoms of the residue in the list
    missing_i: np.ndarray              # [paired residues] int32: of those, atoms the model lacks
    residues: List[pdbio.Residue]      # the REFERENCE's residue of each paired position
    model_residues: List[pdbio.Residue]
    unpaired_reference: int
    unpaired_model: int


def _failed(error: str) -> LddtAtomsResult:
    nan = float("nan")
    return LddtAtomsResult(error, 0, 0, 0, 0, (nan, nan, nan, nan), nan, nan, nan, 0, np.zeros(0, np.int64), np.zeros(0, np.float64),
                           np.zeros(0, np.uint8), np.zeros(0, np.int32), np.zeros(0, np.int32), [], [], 0, 0)


def _score(rows: np.ndarray) -> float:
    total = rows.astype(np.int64).sum(axis=0)
    return fractions(total)[1]


def result_of(lists: AtomLists, rows: np.ndarray, swapped: np.ndarray, totals: np.ndarray, reference_residues, model_residues,
              unpaired_reference: int = 0, unpaired_model: int = 0) -> LddtAtomsResult:
    """One pair's result from its rows of ``atom_out`` and ``swapped_out`` and its row of ``pair_out``."""
    preserved, whole = fractions(totals[2:7])
    n = len(reference_residues)
    n_i, lddt_i = np.zeros(n, np.int64), np.full(n, np.nan)
    flipped, atoms_i, missing_i = np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros(n, np.int32)
    if len(lists.residue):
        starts = np.flatnonzero(np.diff(lists.residue, prepend=-1))
        sums = np.add.reduceat(rows.astype(np.int64), starts, axis=0)
        n_i[lists.residue_at] = sums[:, 0]
        with np.errstate(invalid="ignore", divide="ignore"):
            lddt_i[lists.residue_at] = np.where(sums[:, 0] > 0, sums[:, 1:5].sum(axis=1) / (4.0 * sums[:, 0]), np.nan)
        flipped[lists.residue_at] = np.maximum.reduceat(swapped, starts)
        atoms_i[lists.residue_at] = np.add.reduceat(np.ones(len(lists.residue), np.int32), starts)
        absent = np.isfinite(lists.ref_xyz).all(axis=1) & ~np.isfinite(lists.mob_xyz).all(axis=1)
        missing_i[lists.residue_at] = np.add.reduceat(absent.astype(np.int32), starts)
    return LddtAtomsResult(None, int(totals[0]), int(totals[1]), lists.n_mismatched_residues, int(totals[2]), preserved, whole,
                           _score(rows[lists.backbone]), _score(rows[~lists.backbone]), int(totals[7]), n_i, lddt_i, flipped, atoms_i, missing_i,
                           list(reference_residues), list(model_residues), unpaired_reference, unpaired_model)


def lddt_atoms(pairs: Sequence[Tuple], pair_by: str = "position", symmetry: bool = True, radius: float = RADIUS,
               thresholds: Sequence[float] = THRESHOLDS, device: int = 0, workers: int = 8, budget_bytes: int = structure.BATCH_BYTES,
               stats: Optional[dict] = None) -> List[LddtAtomsResult]:
    """Every ``(reference, model)`` pair — paths of PDB files (plain or gzipped), ``pdbio.Model`` objects or ``AtomLayout`` objects, as
    for ``superpose.superpose``, or what ``superpose.prepare`` / ``cealign.prepare_aligned`` returned — scored under the rule of the
    module docstring.  One GPU call per batch; batches are cut by ``batching.cut_batches`` under ``budget_bytes`` (77 bytes per ATOM:
    its coordinates, indices and counts, nothing per pair of atoms).  A pair that cannot be scored carries its ``error`` and does
    not stop the others.  ``stats`` receives ``submissions``, ``kernel_ms`` and ``files_parsed``."""
    prepared = prepare(pairs, pair_by, "CA", workers)
    lists = {}

    def lists_of(ref, mod, ours, theirs) -> AtomLists:
        key = (id(ref), id(mod), id(ours))
        if key not in lists:
            lists[key] = atom_lists([ref.residues[i] for i in ours], [mod.residues[t] for t in theirs])
        return lists[key]

    def arrays(ref_xyz, mob_xyz, offsets, timing, part):
        mine = [lists_of(*item) for item in part]
        atom_offsets = np.zeros(len(mine) + 1, np.int64)
        np.cumsum([len(one.residue) for one in mine], out=atom_offsets[1:])
        flat = [np.concatenate([getattr(one, field) for one in mine]) for field in ("ref_xyz", "mob_xyz", "residue", "partner")]
        return lddt_atoms_arrays(*flat, atom_offsets, radius, thresholds, symmetry, device, timing), atom_offsets

    def result(got, j, a, b, ref, mod, ours, theirs):
        (tables, atom_offsets), mine = got, lists_of(ref, mod, ours, theirs)
        lo, hi = int(atom_offsets[j]), int(atom_offsets[j + 1])
        return result_of(mine, tables.atom[lo:hi], tables.swapped[lo:hi], tables.pair[j], [ref.residues[i] for i in ours],
                         [mod.residues[t] for t in theirs], len(ref.residues) - len(ours), len(mod.residues) - len(theirs))
    return score_pairs(prepared, budget_bytes, stats, _ATOM_BYTES, arrays, result, _failed,
                       cost=lambda ref, mod, ours, theirs: len(lists_of(ref, mod, ours, theirs).residue), whole_pairs=True)


def layout_of_residues(residues: Sequence[pdbio.Residue]) -> AtomLayout:
    """residues that are already in memory (a built or packed model and its native) as ``lddt_atoms`` takes them"""
    residues = [r for r in residues if not r.hetero]
    return AtomLayout(np.zeros((len(residues), 3)), residues)


def score_models(natives: Sequence[Sequence[pdbio.Residue]], models: Sequence[Sequence[pdbio.Residue]], **keywords) -> List[LddtAtomsResult]:
    """Built or packed models against their natives, residues paired by chain and residue number."""
    return lddt_atoms([(layout_of_residues(a), layout_of_residues(b)) for a, b in zip(natives, models)], pair_by="number", **keywords)


def write_csv(model_path, residue_path, labels: Sequence[Tuple[str, str, str]], results: Sequence[LddtAtomsResult]) -> None:
    """The two files of the command lines: ``labels`` holds (label, reference, model) of each result."""
    with open(model_path, "w", newline="") as fs, open(residue_path, "w", newline="") as fr:
        ws, wr = csv.writer(fs), csv.writer(fr)
        ws.writerow(MODEL_COLUMNS)
        wr.writerow(RESIDUE_COLUMNS)
        for (label, ref, model), res in zip(labels, results):
            ws.writerow([label, str(ref), str(model), res.n_atoms, res.n_missing, res.n_mismatched_residues, res.n_included, _fmt(res.lddt)]
                        + [_fmt(p) for p in res.preserved] + [_fmt(res.lddt_backbone), _fmt(res.lddt_sidechain), res.n_swapped_residues,
                                                             res.error or ""])
            for k, (r, m) in enumerate(zip(res.residues, res.model_residues)):
                wr.writerow([label, r.chain, r.number, r.name, m.name, int(res.atoms_i[k]), int(res.missing_i[k]), int(res.n_i[k]),
                             _fmt(res.lddt_i[k]), int(res.swapped[k])])
