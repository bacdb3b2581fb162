"""Side chains from rotamer classes, batched on the GPU: the inverse of ``structure.tag_rotamers``.  Given the backbone (N, CA, C), a
residue type and chi angles per residue, every side-chain heavy atom is placed by internal coordinates (th_build_sidechains,
csrc/sidechains.hip); the result is measured against the native side chains (per-residue RMSD over atoms of the same name) and
for steric clashes (pairs of atoms of different residues closer than ``clash_distance``).

    *** PARITY UNPINNED AGAINST SCWRL4 ***  The reference gets side chains from SCWRL4 (analyse_rotamers.py analyses 2 and 3,
    ``pack_sidechains``), which chooses rotamers by an energy search and is not available where this project is built.  Nothing
    is searched here: the rotamer is the caller's — a predicted class, the native class, the native angles.  The tree of internal
    coordinates (``sidechain_table``; csrc/sidechain_table.h), its values (standard stereochemistry after Engh & Huber 1991, the
    offsets of the sp3 branches from the means of 1ubq) and the rules, written out in include/timed_hip.h, are this project's own:

    * CB is always built, on (C, N, CA), never copied: a backbone-only model and a mutated position work the same way;
    * ``chi="class_centres"`` builds bin 1 / 2 / 3 at 60 / 180 / -60 degrees; given ``classes`` the residue TYPE comes from the
      class too, so a predicted mutation is built as the predicted residue;
    * unbuilt (all atoms NaN, ``n_built`` 0): a residue that is not one of the 20, GLY, an unlabelled class, a backbone atom or a
      needed chi angle that is missing, N, CA, C on a line;
    * the RMSD pairs atoms BY NAME with the native residue where it is of the built type, without symmetry correction: a ring or
      carboxylate deposited the other way round (chi2 off by 180 degrees) is reported as named;
    * a clash is a side-chain atom closer than ``clash_distance`` (default 2.5 Angstrom, strict) to an atom of another residue of
      the structure — built side-chain atoms and N, CA, C, O —, except the backbone of a chain neighbour and SG-SG pairs.  There
      are no radii and no hydrogens.

Rebuilding 1ubq from its native chi angles gives 0.347 Angstrom over its 297 side-chain heavy atoms (tests/golden/
make_sidechain_golden.py).
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib, batching, pdbio, structure
from ._lib import ptr

MAX_ATOMS = 10
CLASH_DISTANCE = 2.5
BIN_CENTRES = (60.0, 180.0, -60.0)        # bins 1, 2, 3 of th_tag_rotamers
BACKBONE = ("N", "CA", "C", "O")
TH_SC_BACKBONE_O = 1
BATCH_BYTES = batching.BATCH_BYTES
_RES_BYTES = 640                          # host bytes per residue of one call: inputs, outputs and about eight native atoms
_LANES = ("N", "CA", "C")


@dataclass
class SidechainType:
    res: str                                                   # three-letter code
    atoms: Tuple[str, ...]                                     # side-chain heavy atoms in build order
    parents: Tuple[Tuple[str, str, str], ...]                  # a, b, c of each atom: d is bonded to c
    chi_index: Tuple[int, ...]                                 # k: the dihedral a-b-c-d is chi[k] + offset, the offset alone for -1
    geometry: Tuple[Tuple[float, float, float], ...]           # |cd| in Angstrom, angle b-c-d and dihedral offset in degrees
    closure: Tuple[Tuple[str, str, float], ...]                # ring bonds the tree does not use, with the length stated for each


_TABLE: Optional[List[SidechainType]] = None


def sidechain_table() -> List[SidechainType]:
    """th_sidechain_table for the 20 residue types in the codec's order.  Host code, no GPU needed."""
    global _TABLE
    if _TABLE is None:
        from design_utils.amino_acids import standard_amino_acids
        lib, rows = _lib.load(), []
        for t, res in enumerate(standard_amino_acids.values()):
            n, n_closure = C.c_int(0), C.c_int(0)
            names = C.create_string_buffer(4 * MAX_ATOMS)
            parents, chi_index = np.zeros((MAX_ATOMS, 3), np.int8), np.zeros(MAX_ATOMS, np.int8)
            geometry, closure_atoms, closure_length = np.zeros((MAX_ATOMS, 3)), np.zeros((2, 2), np.int8), np.zeros(2)
            _lib.check(lib.th_sidechain_table(t, C.byref(n), names, ptr(parents), ptr(chi_index), ptr(geometry), C.byref(n_closure),
                                              ptr(closure_atoms), ptr(closure_length)))
            atoms = tuple(names.raw[4 * j:4 * j + 4].rstrip(b"\0").decode("ascii") for j in range(n.value))
            lanes = _LANES + atoms
            rows.append(SidechainType(res, atoms, tuple(tuple(lanes[p] for p in parents[j]) for j in range(n.value)),
                                      tuple(int(k) for k in chi_index[:n.value]), tuple(tuple(float(x) for x in geometry[j]) for j in range(n.value)),
                                      tuple((atoms[closure_atoms[q, 0]], atoms[closure_atoms[q, 1]], float(closure_length[q]))
                                            for q in range(n_closure.value))))
        _TABLE = rows
    return _TABLE


def class_centres(classes) -> Tuple[np.ndarray, np.ndarray]:
    """Rotamer class indices (-1: unlabelled) -> (int8 [n] residue types, float64 [n, 4] chi angles at the centres of the class's
    bins: 60 / 180 / -60 degrees for bins 1 / 2 / 3, NaN beyond the type's angles).  An unlabelled class gives type -1."""
    classes = np.asarray(classes, dtype=np.int64).reshape(-1)
    table = structure.rotamer_table()
    bases = np.array([base for _, _, base, _ in table], dtype=np.int64)
    n_classes = int(bases[-1] + 3 ** table[-1][1])
    if ((classes < -1) | (classes >= n_classes)).any():
        raise ValueError(f"rotamer classes run from -1 to {n_classes - 1}")
    types = (np.searchsorted(bases, classes, side="right") - 1).astype(np.int8)
    types[classes < 0] = -1
    chi = np.full((classes.size, 4), np.nan)
    centres = np.array(BIN_CENTRES)
    for r in np.flatnonzero(classes >= 0):
        n_chi, index = table[types[r]][1], int(classes[r] - bases[types[r]])
        for k in range(n_chi - 1, -1, -1):                     # the first angle varies slowest
            chi[r, k] = centres[index % 3]
            index //= 3
    return types, chi


@dataclass
class BuiltArrays:
    xyz: np.ndarray                        # [n_res, 10, 3] float64, NaN beyond n_built
    n_built: np.ndarray                    # [n_res] int32
    n_matched: Optional[np.ndarray]        # [n_res] int32, with a native
    sum_sq: Optional[np.ndarray]           # [n_res] float64, with a native
    clashes: Optional[np.ndarray]          # [n_res] int32
    pairs: Optional[np.ndarray]            # [n_struct] int64


def build_arrays(backbone, res_type, chi, struct_offsets=None, chain_id=None, native=None, clash_distance: float = CLASH_DISTANCE,
                 clashes: bool = True, device: int = 0, timing: Optional[dict] = None) -> BuiltArrays:
    """One th_build_sidechains call on flat arrays.  ``backbone`` [n_res, 3 or 4, 3] (N, CA, C and optionally O), ``res_type``
    [n_res] (-1..19), ``chi`` [n_res, 4] degrees, ``struct_offsets`` [S + 1] (default: one structure), ``chain_id`` [n_res] or
    None (one chain), ``native`` None or (xyz [total, 3], packed names [total], res_offsets [n_res + 1], types [n_res]) as
    ``structure.rotamer_classes`` takes them.  ``timing``: a dict whose ``kernel_ms`` grows by the device time of the kernels."""
    backbone = np.ascontiguousarray(backbone, dtype=np.float64)
    res_type = np.ascontiguousarray(res_type, dtype=np.int8).reshape(-1)
    n_res = res_type.size
    if backbone.ndim != 3 or backbone.shape[0] != n_res or backbone.shape[1] not in (3, 4) or backbone.shape[2] != 3:
        raise ValueError(f"backbone needs the shape [{n_res}, 3 or 4, 3]")
    chi = np.ascontiguousarray(chi, dtype=np.float64).reshape(-1, 4)
    if chi.shape[0] != n_res:
        raise ValueError(f"chi needs {n_res} rows of four angles")
    offsets = np.ascontiguousarray([0, n_res] if struct_offsets is None else struct_offsets, dtype=np.int64).reshape(-1)
    if offsets.size < 1:
        raise ValueError("struct_offsets needs at least one entry")
    if chain_id is not None:
        chain_id = np.ascontiguousarray(chain_id, dtype=np.int32).reshape(-1)
        if chain_id.size != n_res:
            raise ValueError(f"chain_id needs {n_res} entries")
    n_total, n_xyz, n_name, n_off, n_type, n_matched, sum_sq = 0, None, None, None, None, None, None
    if native is not None:
        n_xyz = np.ascontiguousarray(native[0], dtype=np.float64).reshape(-1, 3)
        n_name = np.ascontiguousarray(native[1], dtype=np.uint32).reshape(-1)
        n_off = np.ascontiguousarray(native[2], dtype=np.int64).reshape(-1)
        n_type = np.ascontiguousarray(native[3], dtype=np.int8).reshape(-1)
        n_total = n_xyz.shape[0]
        if n_name.size != n_total or n_off.size != n_res + 1 or n_type.size != n_res:
            raise ValueError(f"the native needs {n_total} names, {n_res + 1} residue offsets and {n_res} types")
        n_matched, sum_sq = np.zeros(n_res, np.int32), np.zeros(n_res, np.float64)
    xyz = np.full((n_res, MAX_ATOMS, 3), np.nan)
    n_built = np.zeros(n_res, np.int32)
    counts = np.zeros(n_res, np.int32) if clashes else None
    pairs = np.zeros(offsets.size - 1, np.int64) if clashes else None
    ms = C.c_double(0.0)
    _lib.check(_lib.load().th_build_sidechains(
        int(device), ptr(backbone), ptr(res_type), ptr(chi), ptr(chain_id), ptr(offsets), offsets.size - 1, n_res, ptr(n_xyz), ptr(n_name),
        n_total, ptr(n_off), ptr(n_type), float(clash_distance), TH_SC_BACKBONE_O if backbone.shape[1] == 4 else 0, ptr(xyz), ptr(n_built),
        ptr(n_matched), ptr(sum_sq), ptr(counts), ptr(pairs), C.byref(ms) if timing is not None else None))
    if timing is not None:
        timing["kernel_ms"] = timing.get("kernel_ms", 0.0) + ms.value
    return BuiltArrays(xyz, n_built, n_matched, sum_sq, counts, pairs)


@dataclass
class SidechainLayout:
    """One structure as th_build_sidechains takes it."""
    native: structure.RotamerLayout        # the native atoms, residue after residue (non-hetero residues, chains in file order)
    backbone: np.ndarray                   # [n, 4, 3] float64: N, CA, C, O, NaN where the residue lacks the atom
    chain_id: np.ndarray                   # [n] int32: chains numbered in file order
    res_type: np.ndarray                   # [n] int8: the type to build
    chi: np.ndarray                        # [n, 4] float64: the angles to build with
    cls: Optional[np.ndarray] = None       # [n] int16: the class the angles came from, when they came from one

    @property
    def residues(self) -> List[pdbio.Residue]:
        return self.native.residues


def backbone_of(residues: Sequence[pdbio.Residue]) -> Tuple[np.ndarray, np.ndarray]:
    """([n, 4, 3] N, CA, C, O with NaN for an absent atom, [n] int32 chain numbers in order of first appearance)"""
    backbone = np.full((len(residues), 4, 3), np.nan)
    chains: dict = {}
    chain_id = np.zeros(len(residues), np.int32)
    for r, res in enumerate(residues):
        for a, name in enumerate(BACKBONE):
            if name in res.atoms:
                backbone[r, a] = res.atoms[name]
        chain_id[r] = chains.setdefault(res.chain, len(chains))
    return backbone, chain_id


@dataclass
class BuiltSidechains:
    residues: List[pdbio.Residue]          # the native residues, chains in file order
    built_names: List[Optional[str]]       # the residue built at each position (three-letter code), None for type -1
    atom_names: List[Tuple[str, ...]]      # the names of the n_built atoms of each residue, in build order
    xyz: np.ndarray                        # [n, 10, 3] float64, NaN beyond n_built
    n_built: np.ndarray                    # [n] int32
    n_matched: np.ndarray                  # [n] int32: built atoms that found a native atom of their name
    sum_sq: np.ndarray                     # [n] float64: their summed squared deviation
    clashes: np.ndarray                    # [n] int32
    pairs: int                             # clashing pairs of the structure, each once
    chi: np.ndarray                        # [n, 4] float64: the angles used
    cls: Optional[np.ndarray]              # [n] int16 or None
    backbone: np.ndarray                   # [n, 4, 3]

    @property
    def rmsd(self) -> np.ndarray:
        """per-residue side-chain RMSD in Angstrom, NaN where nothing matched"""
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.n_matched > 0, np.sqrt(self.sum_sq / self.n_matched), np.nan)

    @property
    def overall_rmsd(self) -> float:
        n = int(self.n_matched.sum())
        return float(np.sqrt(self.sum_sq.sum() / n)) if n else float("nan")

    def to_model(self) -> pdbio.Model:
        """N, CA, C, O of the native (with their B-factors) and the built side chains (B-factor 0), under the BUILT residue names"""
        out = []
        for r, res in enumerate(self.residues):
            new = pdbio.Residue(res.chain, res.number, self.built_names[r] or res.name)
            for name in BACKBONE:
                if name in res.atoms:
                    new.atoms[name] = np.asarray(res.atoms[name], dtype=np.float64)
                    new.elements[name] = name[0]
                    new.bfactors[name] = res.bfactors.get(name, float("nan"))
            for j, name in enumerate(self.atom_names[r]):
                new.atoms[name] = self.xyz[r, j].copy()
                new.elements[name] = name[0]
                new.bfactors[name] = 0.0
            out.append(new)
        return pdbio.Model(1, out)


def build_layouts(layouts: Sequence[SidechainLayout], clash_distance: float = CLASH_DISTANCE, device: int = 0,
                  budget_bytes: int = BATCH_BYTES, stats: Optional[dict] = None) -> List[BuiltSidechains]:
    """The layouts through th_build_sidechains in as few calls as ``budget_bytes`` allows.  ``stats`` receives ``submissions`` and
    ``kernel_ms``."""
    from design_utils.amino_acids import standard_amino_acids
    names, table = list(standard_amino_acids.values()), sidechain_table()
    out: List[BuiltSidechains] = []

    def submit(part, timing):
        res_lo = np.zeros(len(part) + 1, np.int64)
        np.cumsum([len(l.res_type) for l in part], out=res_lo[1:])
        atom_lo = np.zeros(len(part) + 1, np.int64)
        np.cumsum([len(l.native.xyz) for l in part], out=atom_lo[1:])
        native = (np.concatenate([l.native.xyz for l in part]), np.concatenate([l.native.atom_name for l in part]),
                  np.concatenate([l.native.res_offsets[:-1] + atom_lo[k] for k, l in enumerate(part)] + [atom_lo[-1:]]),
                  np.concatenate([l.native.res_type for l in part]))
        got = build_arrays(np.concatenate([l.backbone for l in part]), np.concatenate([l.res_type for l in part]),
                           np.concatenate([l.chi for l in part]), res_lo, np.concatenate([l.chain_id for l in part]), native,
                           clash_distance, True, device, timing)
        for k, l in enumerate(part):
            lo, hi = res_lo[k], res_lo[k + 1]
            n_built = got.n_built[lo:hi].copy()
            out.append(BuiltSidechains(
                l.residues, [names[t] if t >= 0 else None for t in l.res_type.tolist()],
                [table[t].atoms if n else () for t, n in zip(l.res_type.tolist(), n_built.tolist())], got.xyz[lo:hi].copy(), n_built,
                got.n_matched[lo:hi].copy(), got.sum_sq[lo:hi].copy(), got.clashes[lo:hi].copy(), int(got.pairs[k]), l.chi, l.cls, l.backbone))
    batching.run_batches(layouts, [len(l.res_type) for l in layouts], budget_bytes, _RES_BYTES, submit, stats)
    return out


def cut_batches(sizes: Sequence[int], budget_bytes: int = BATCH_BYTES) -> List[Tuple[int, int]]:
    """[lo, hi) runs of consecutive structures whose residues fit ``budget_bytes`` (a structure above it goes alone)."""
    return batching.cut_batches(sizes, budget_bytes, _RES_BYTES)


def build(structures: Sequence[Union[pdbio.Model, structure.RotamerLayout, str, os.PathLike]], chi="native", classes=None, types=None,
          clash_distance: float = CLASH_DISTANCE, device: int = 0, budget_bytes: int = BATCH_BYTES,
          stats: Optional[dict] = None) -> List[BuiltSidechains]:
    """Side chains of every structure (``pdbio.Model`` objects, ``RotamerLayout`` objects or paths of PDB files) on its native
    backbone, under the rules of the module docstring.

    ``chi``: ``"native"`` — the chi angles of the structure itself (``structure.tag_rotamers``); ``"class_centres"`` — the centres
    of the bins of ``classes`` (per structure an array of class indices, -1 unlabelled), or of the native classes when ``classes``
    is None; or per structure an array [residues, 4] of angles in degrees.
    ``types``: per structure an array of residue types (-1..19) to build; default: the type of the class where ``classes`` is
    given (a predicted mutation is built as the predicted residue), else the native type.
    One GPU call per batch, cut by ``budget_bytes``; ``stats`` receives ``submissions`` and ``kernel_ms`` of the building calls."""
    natives = [s if isinstance(s, structure.RotamerLayout) else structure.rotamer_layout(structure.first_model(s)) for s in structures]
    if classes is not None and len(classes) != len(natives) or types is not None and len(types) != len(natives):
        raise ValueError(f"classes and types need one entry per structure ({len(natives)})")
    by_name = isinstance(chi, str)
    if by_name and chi not in ("native", "class_centres"):
        raise ValueError(f"chi is \"native\", \"class_centres\" or one array per structure, not {chi!r}")
    if not by_name and len(chi) != len(natives):
        raise ValueError(f"chi needs one array per structure ({len(natives)})")
    if classes is not None and chi == "native":
        raise ValueError("classes are built at their centres: chi=\"class_centres\"")
    tagged = None
    if by_name and (chi == "native" or classes is None):
        tagged = structure.tag_rotamers(natives, device=device, budget_bytes=budget_bytes)
    layouts = []
    for s, native in enumerate(natives):
        n = len(native.residues)
        backbone, chain_id = backbone_of(native.residues)
        cls, res_type = None, native.res_type
        if by_name and chi == "class_centres":
            cls = np.asarray(tagged[s].cls if classes is None else classes[s], dtype=np.int16).reshape(-1)
            if cls.size != n:
                raise ValueError(f"structure {s} has {n} residues and {cls.size} classes")
            res_type, angles = class_centres(cls)
        elif by_name:
            angles = tagged[s].chi
        else:
            angles = np.asarray(chi[s], dtype=np.float64).reshape(-1, 4)
        if types is not None:
            res_type = np.asarray(types[s], dtype=np.int8).reshape(-1)
        if len(res_type) != n or len(angles) != n:
            raise ValueError(f"structure {s} has {n} residues, {len(res_type)} types and {len(angles)} rows of chi angles")
        layouts.append(SidechainLayout(native, backbone, chain_id, np.ascontiguousarray(res_type, dtype=np.int8),
                                       np.ascontiguousarray(angles, dtype=np.float64), cls))
    return build_layouts(layouts, clash_distance, device, budget_bytes, stats)
