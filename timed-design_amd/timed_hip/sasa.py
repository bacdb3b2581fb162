"""Solvent-accessible surface area (SASA) of PDB structures, batched on the GPU: which atoms and residues are buried and which face the
solvent, by the numerical method of Shrake & Rupley (1973), through th_sasa (csrc/sasa.hip): every atom carries a sphere of its van
der Waals radius plus the probe radius with test points on it, and a point is exposed unless it lies inside the sphere of another
atom; every structure of a batch in one call.  How much hydrophobic surface a design leaves in the solvent, and which residues are
core, boundary and surface.  The reference has only its contact number (``timed_hip.structure.packing_density``) for this.

    *** PARITY UNPINNED AGAINST FREESASA / NACCESS / DSSP / BIOPYTHON ***  None of them is available where this project is built
    (verified absent: the Python modules ``Bio``, ``freesasa`` and ``mdtraj``).  The rule is this project's own; it is written out in
    include/timed_hip.h.  Those programs use their own radii, point sets or slices and tie rules: areas differ in detail.

    Per structure, atoms 0 .. n-1 in file order, each with xyz and a van der Waals radius (float64); the call takes a ``probe`` and
    ``n_points`` direction vectors u_k (normally ``sphere_points``: the golden spiral).  Every float64 product, sum and difference is
    rounded on its own, in the written order:

    * expanded radius: R_i = radius_i + probe;
    * valid(i): the three coordinates and R_i are finite and R_i > 0.  An invalid atom occludes nothing, its count is -1, its mask
      words are 0 and its area is 0;
    * near(i, j): j != i, the same structure, both valid, and s < t*t, strict, with s = (dx*dx + dy*dy) + dz*dz, dx = x_j - x_i ...,
      t = R_i + R_j.  The pre-filter is part of the rule: an atom that is not near occludes nothing;
    * sphere points: p_k = (x_i + R_i*u_kx, y_i + R_i*u_ky, z_i + R_i*u_kz);
    * occlusion: point k of atom i is buried iff some j with near(i, j) has (ex*ex + ey*ey) + ez*ez < R_j*R_j, strict, with
      e = p_k - c_j.  A point exactly on a neighbour's sphere is exposed;
    * count: exposed[i] = the number of points not buried (int32); mask[i][w] bit b = point 64 w + b exposed, padding bits 0;
    * structure totals (int64 [S, 3]): valid atoms, valid atoms with exposed == 0, the sum of exposed over valid atoms;
    * areas, on the host in float64: area_i = exposed_i * (4 * pi * R_i * R_i / n_points), multiplied left to right; a residue's area
      is the sequential sum over its atoms in file order.  Polar = N and O atoms, apolar = everything else, backbone = the atoms
      named N, CA, C and O.

    Consequences: coincident atoms of equal radius bury each other's points only as far as the rounding of |u_k| decides
    (deterministic, physically meaningless); a sphere wholly inside another gets 0; distances that overflow to infinity are not near;
    ``probe = 0`` gives the van der Waals surface.

The atoms (``atom_layout``): the first model, the first alternate location, the non-hydrogen atoms (``structure.is_hydrogen``) of the
non-hetero residues of ALL chains, in file order.  ``include_hetero=True``: the non-water hetero atoms also occlude and are reported
per atom, under no residue.  Waters (HOH, WAT, DOD) never occlude.  Radii go by element — the element column, else the first letter of
the atom name — from ``design_utils.amino_acids.vdw_radii`` (Bondi: C 1.70, N 1.55, O 1.52, S 1.80, P 1.80, SE 1.90, anything else
1.80), or from the caller's dict.

Relative accessibility: rsa = area / ``design_utils.amino_acids.max_asa``[residue name] (after Tien et al. 2013, theoretical; that
table is WRITTEN FROM MEMORY, NOT FETCHED), not clamped — a chain end can exceed 1; NaN for a residue outside the table.  Burial
classes, a convention and not a measurement: 0 core (rsa < ``core`` = 0.2), 2 surface (rsa >= ``surface`` = 0.5), 1 boundary, -1 unknown.

``interface=True``: a structure of more than one chain is additionally submitted chain by chain, as further structures of the same
batch; per residue the area lost in the complex is reported, per structure the buried interface area, the sum over the chains alone
minus the complex.

Out of scope: Lee-Richards slices, per-atom-type radius sets (ProtOr, NACCESS), explicit hydrogens, analytic surfaces and volumes, NMR
ensembles, a cell grid for the neighbour search (all pairs per structure, as every sibling kernel).
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib, batching, pdbio, structure
from ._lib import ptr

MAX_POINTS = 1024
BURIAL_LETTERS = "CBS"                 # the letter of burial classes 0, 1, 2; "?" for -1
_BACKBONE = ("N", "CA", "C", "O")
_ATOM_BYTES = 3 * 8 + 8 + 4            # xyz, radius, exposed


class SasaTables(NamedTuple):
    """What one th_sasa call returns."""
    exposed: np.ndarray                # [total] int32: exposed points, -1 for an invalid atom
    mask: Optional[np.ndarray]         # [total, ceil(n_points / 64)] uint64, or None when not asked for
    structure: np.ndarray              # [S, 3] int64: valid atoms, valid atoms without an exposed point, the sum of exposed


def mask_words(n_points: int) -> int:
    return (int(n_points) + 63) // 64


def atom_bytes(n_points: int, mask: bool = False) -> int:
    """what one atom takes in one call: 32 bytes in, 4 out, and 8 per 64 points when the mask is asked for"""
    return _ATOM_BYTES + (8 * mask_words(n_points) if mask else 0)


def sphere_points(n: int) -> np.ndarray:
    """[n, 3] float64: the golden spiral of th_sasa_sphere (host code, no GPU needed), 1 <= n <= 1024"""
    out = np.empty((max(int(n), 0), 3), np.float64)
    _lib.check(_lib.load().th_sasa_sphere(int(n), ptr(out)))
    return out


def sasa_arrays(xyz, radius, offsets, probe: float = 1.4, points=None, n_points: int = 96, device: int = 0, mask: bool = False,
                timing: Optional[dict] = None) -> SasaTables:
    """One th_sasa call.  ``xyz`` [total, 3] float64, ``radius`` [total] float64, ``offsets`` [S + 1]; ``points`` [n, 3] or None for
    ``sphere_points(n_points)``.  ``mask``: also return which points are exposed.  ``timing``: a dict whose ``kernel_ms`` grows by the
    device time of the kernels and whose ``points_ms`` and ``totals_ms`` grow by that of each."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    radius = np.ascontiguousarray(radius, dtype=np.float64).reshape(-1)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    if offsets.size < 1:
        raise ValueError("offsets needs at least one entry")
    total, n_structures = xyz.shape[0], offsets.size - 1
    if radius.size != total:
        raise ValueError(f"radius needs {total} entries")
    points = sphere_points(n_points) if points is None else np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    n = points.shape[0]
    exposed = np.empty(total, np.int32)
    words = np.empty((total, mask_words(n)), np.uint64) if mask else None
    per_structure = np.empty((n_structures, 3), np.int64)
    ms = (C.c_double * 2)(0.0, 0.0)
    _lib.check(_lib.load().th_sasa(int(device), ptr(xyz), ptr(radius), total, ptr(offsets), n_structures, float(probe), ptr(points), n,
                                   ptr(exposed), ptr(words), ptr(per_structure),
                                   C.cast(ms, C.POINTER(C.c_double)) if timing is not None else None))
    if timing is not None:
        timing["kernel_ms"] = timing.get("kernel_ms", 0.0) + sum(ms)
        for key, value in zip(("points_ms", "totals_ms"), ms):
            timing[key] = timing.get(key, 0.0) + value
    return SasaTables(exposed, words, per_structure)


def atom_areas(exposed, radius, probe: float, n_points: int) -> np.ndarray:
    """area_i = exposed_i * (4 pi R_i R_i / n_points) with R_i = radius_i + probe, multiplied left to right; 0 for an invalid atom"""
    exposed = np.asarray(exposed, dtype=np.int64)
    R = np.asarray(radius, dtype=np.float64) + float(probe)
    unit = 4.0 * math.pi * R * R / float(n_points)
    return np.where(exposed >= 0, exposed.astype(np.float64) * unit, 0.0)


def element_of(name: str, element: str) -> str:
    """the element column in upper case; where it is absent or no letter, the first letter of the atom name behind any digits"""
    el = element.strip().upper()
    if not el or not el[0].isalpha():
        el = name.lstrip("0123456789 ").upper()[:1]
    return el


def _radii(radii: Optional[Dict[str, float]]):
    from design_utils.amino_acids import VDW_RADIUS_OTHER, vdw_radii
    return (vdw_radii if radii is None else radii), VDW_RADIUS_OTHER


def is_water(res: pdbio.Residue) -> bool:
    from design_utils.amino_acids import WATER_NAMES
    return res.name in WATER_NAMES


@dataclass
class AtomLayout:
    """One structure as th_sasa takes it."""
    xyz: np.ndarray                    # [n, 3] float64, file order
    radius: np.ndarray                 # [n] float64: van der Waals radii
    group: np.ndarray                  # [n] int32: index into ``residues``, -1 for a hetero atom
    polar: np.ndarray                  # [n] bool: N and O atoms
    backbone: np.ndarray               # [n] bool: N, CA, C, O of a reported residue
    atoms: List[Tuple[pdbio.Residue, str]]     # per atom: its residue and its name
    residues: List[pdbio.Residue]      # the reported residues: non-hetero, every chain, file order


def layout_of_residues(residues: Sequence[pdbio.Residue], radii: Optional[Dict[str, float]] = None) -> AtomLayout:
    """The non-hydrogen atoms of the residues as they come; a hetero residue's atoms belong to no reported residue."""
    table, other = _radii(radii)
    xyz, radius, group, polar, backbone, atoms, reported = [], [], [], [], [], [], []
    for res in residues:
        g = -1
        if not res.hetero:
            g = len(reported)
            reported.append(res)
        for name, pos in res.atoms.items():
            if structure.is_hydrogen(name, res.elements.get(name, "")):
                continue
            el = element_of(name, res.elements.get(name, ""))
            xyz.append(pos)
            radius.append(float(table.get(el, other)))
            group.append(g)
            polar.append(el in ("N", "O"))
            backbone.append(g >= 0 and name in _BACKBONE)
            atoms.append((res, name))
    return AtomLayout(np.array(xyz, dtype=np.float64).reshape(-1, 3), np.array(radius, dtype=np.float64), np.array(group, dtype=np.int32),
                      np.array(polar, dtype=bool), np.array(backbone, dtype=bool), atoms, reported)


def atom_layout(model: pdbio.Model, include_hetero: bool = False, radii: Optional[Dict[str, float]] = None) -> AtomLayout:
    """Apply the atom rule (module docstring) to one model."""
    return layout_of_residues([r for r in model.residues if not r.hetero or (include_hetero and not is_water(r))], radii)


def chain_layouts(layout: AtomLayout) -> List[Tuple[str, np.ndarray, AtomLayout]]:
    """(chain, indices of its atoms in ``layout``, the chain alone as a layout) for every chain of the layout, in order of appearance"""
    chains: Dict[str, List[int]] = {}
    for k, (res, _) in enumerate(layout.atoms):
        chains.setdefault(res.chain, []).append(k)
    out = []
    for chain, members in chains.items():
        idx = np.array(members, dtype=np.int64)
        old = layout.group[idx]
        kept = [g for g in dict.fromkeys(old.tolist()) if g >= 0]
        renumber = {g: k for k, g in enumerate(kept)}
        group = np.array([renumber.get(g, -1) for g in old.tolist()], dtype=np.int32)
        out.append((chain, idx, AtomLayout(layout.xyz[idx], layout.radius[idx], group, layout.polar[idx], layout.backbone[idx],
                                           [layout.atoms[k] for k in members], [layout.residues[g] for g in kept])))
    return out


@dataclass
class StructureSasa:
    error: Optional[str]               # why the structure was not measured (everything below is then empty / 0)
    exposed: np.ndarray                # [atoms] int32: exposed points, -1 for an invalid atom
    area: np.ndarray                   # [atoms] float64, Angstrom^2
    radius: np.ndarray                 # [atoms] float64: the van der Waals radius used
    atoms: List[Tuple[pdbio.Residue, str]]     # per atom: its residue and its name
    mask: Optional[np.ndarray]         # [atoms, words] uint64 when asked for
    residues: List[pdbio.Residue]
    residue_area: np.ndarray           # [residues] float64
    polar_area: np.ndarray             # [residues] float64: N and O atoms
    apolar_area: np.ndarray            # [residues] float64: every other atom
    backbone_area: np.ndarray          # [residues] float64: N, CA, C, O
    rsa: np.ndarray                    # [residues] float64: area / max_asa, NaN for a residue outside the table
    burial: np.ndarray                 # [residues] int8: 0 core, 1 boundary, 2 surface, -1 unknown
    n_atoms: int                       # valid atoms
    n_buried_atoms: int                # valid atoms without an exposed point
    n_exposed_points: int
    total_area: float                  # over all atoms, hetero atoms included when they were asked for
    total_polar_area: float
    total_apolar_area: float
    area_lost: Optional[np.ndarray] = None     # [residues] float64: area in its chain alone minus area in the complex (``interface``)
    interface_area: float = float("nan")       # sum over the chains alone minus the complex; NaN unless ``interface``

    @property
    def counts(self) -> Tuple[int, int, int]:
        """(core, boundary, surface) residues"""
        return tuple(int((self.burial == k).sum()) for k in (0, 1, 2))

    @property
    def apolar_share(self) -> float:
        return self.total_apolar_area / self.total_area if self.total_area > 0 else float("nan")

    @property
    def burial_letters(self) -> str:
        return "".join(BURIAL_LETTERS[b] if b >= 0 else "?" for b in self.burial.tolist())


def _failed(error: str) -> StructureSasa:
    f, i = np.zeros(0, np.float64), np.zeros(0, np.int32)
    return StructureSasa(error, i, f, f, [], None, [], f, f, f, f, f, np.zeros(0, np.int8), 0, 0, 0, 0.0, 0.0, 0.0)


def _sequential(values, keep) -> float:
    total = 0.0
    for v, k in zip(values, keep):
        if k:
            total += v
    return total


def burial_classes(rsa, core: float = 0.2, surface: float = 0.5) -> np.ndarray:
    """int8: 0 where rsa < core, 2 where rsa >= surface, 1 between, -1 where rsa is NaN"""
    rsa = np.asarray(rsa, dtype=np.float64)
    out = np.where(rsa < core, 0, np.where(rsa >= surface, 2, 1)).astype(np.int8)
    out[np.isnan(rsa)] = -1
    return out


def assemble(layout: AtomLayout, exposed, totals, mask, probe: float, n_points: int, core: float = 0.2, surface: float = 0.5) -> StructureSasa:
    """The areas of one structure from the integers of th_sasa: plain loops over the atoms in file order"""
    from design_utils.amino_acids import max_asa
    area = atom_areas(exposed, layout.radius, probe, n_points)
    n_res = len(layout.residues)
    sums = np.zeros((4, n_res), np.float64)    # all, polar, apolar, backbone
    for a, g, p, b in zip(area.tolist(), layout.group.tolist(), layout.polar.tolist(), layout.backbone.tolist()):
        if g < 0:
            continue
        sums[0, g] += a
        sums[1 if p else 2, g] += a
        if b:
            sums[3, g] += a
    largest = np.array([max_asa.get(r.name, float("nan")) for r in layout.residues], dtype=np.float64)
    rsa = sums[0] / largest if n_res else np.zeros(0, np.float64)
    values, polar = area.tolist(), layout.polar.tolist()
    return StructureSasa(None, np.asarray(exposed, np.int32).copy(), area, layout.radius, layout.atoms, None if mask is None else mask.copy(),
                         layout.residues, sums[0], sums[1], sums[2], sums[3], rsa, burial_classes(rsa, core, surface), int(totals[0]),
                         int(totals[1]), int(totals[2]), _sequential(values, [True] * len(values)), _sequential(values, polar),
                         _sequential(values, [not p for p in polar]))


def sasa_layouts(layouts: Sequence[AtomLayout], probe: float = 1.4, points=None, n_points: int = 96, device: int = 0, mask: bool = False,
                 core: float = 0.2, surface: float = 0.5, interface: bool = False, budget_bytes: int = batching.BATCH_BYTES,
                 stats: Optional[dict] = None) -> List[StructureSasa]:
    """The layouts through th_sasa in as few calls as ``budget_bytes`` allows; a structure is charged its atoms and, when ``mask`` is
    asked for, its mask (``atom_bytes``).  ``interface``: the chains of a structure of more than one chain follow it as structures of
    their own.  ``stats`` receives ``submissions`` and ``kernel_ms``."""
    points = sphere_points(n_points) if points is None else np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    n_points = points.shape[0]
    jobs: List[AtomLayout] = []
    alone: List[list] = []                     # per layout: its (chain, atom indices, position in jobs), empty without an interface
    for lay in layouts:
        jobs.append(lay)
        parts = chain_layouts(lay) if interface else []
        parts = parts if len(parts) > 1 else []
        alone.append([(chain, idx, len(jobs) + k) for k, (chain, idx, _) in enumerate(parts)])
        jobs += [part for _, _, part in parts]
    measured: List[StructureSasa] = []

    def submit(part, timing):
        offsets = np.zeros(len(part) + 1, np.int64)
        np.cumsum([len(l.xyz) for l in part], out=offsets[1:])
        got = sasa_arrays(np.concatenate([l.xyz for l in part]), np.concatenate([l.radius for l in part]), offsets, probe, points,
                          device=device, mask=mask, timing=timing)
        for k, l in enumerate(part):
            a, b = int(offsets[k]), int(offsets[k + 1])
            measured.append(assemble(l, got.exposed[a:b], got.structure[k], None if got.mask is None else got.mask[a:b], probe, n_points,
                                     core, surface))
    batching.run_batches(jobs, [len(l.xyz) for l in jobs], budget_bytes, atom_bytes(n_points, mask), submit, stats)
    out, at = [], 0
    for lay, chains in zip(layouts, alone):
        res = measured[at]
        at += 1 + len(chains)
        if interface:
            res.area_lost = np.zeros(len(res.residues), np.float64)
            res.interface_area = 0.0
        if chains:
            index = {id(r): k for k, r in enumerate(res.residues)}
            separate = 0.0
            for _, _, position in chains:
                single = measured[position]
                separate += single.total_area
                for r, a in zip(single.residues, single.residue_area.tolist()):
                    res.area_lost[index[id(r)]] = a - res.residue_area[index[id(r)]]
            res.interface_area = separate - res.total_area
        out.append(res)
    return out


def sasa(files_or_models: Sequence[Union[pdbio.Model, AtomLayout, str, os.PathLike]], probe: float = 1.4, points=None, n_points: int = 96,
         device: int = 0, include_hetero: bool = False, radii: Optional[Dict[str, float]] = None, mask: bool = False, core: float = 0.2,
         surface: float = 0.5, interface: bool = False, budget_bytes: int = batching.BATCH_BYTES, workers: int = 8,
         stats: Optional[dict] = None) -> List[StructureSasa]:
    """The solvent-accessible surface of every structure (``pdbio.Model`` objects, ``AtomLayout`` objects or paths of PDB files, plain
    or gzipped) under the rule of the module docstring.  Files are parsed on ``workers`` host threads; one GPU call per batch, batches
    cut under ``budget_bytes``.  A file that cannot be read carries its ``error`` and does not stop the others.  ``stats`` receives
    ``submissions``, ``kernel_ms`` and ``files_parsed``."""
    def parse(item):
        if isinstance(item, AtomLayout):
            return item
        try:
            return atom_layout(structure.first_model(item), include_hetero, radii)
        except (OSError, EOFError, ValueError) as e:
            return f"{type(e).__name__}: {e}"
    items = list(files_or_models)
    parsed = batching.parse_each(parse, items, workers)
    good = [p for p in parsed if not isinstance(p, str)]
    if stats is not None:
        stats["files_parsed"] = stats.get("files_parsed", 0) + sum(1 for item in items if not isinstance(item, (AtomLayout, pdbio.Model)))
    measured = iter(sasa_layouts(good, probe, points, n_points, device, mask, core, surface, interface, budget_bytes, stats))
    return [_failed(p) if isinstance(p, str) else next(measured) for p in parsed]
