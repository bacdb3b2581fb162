"""Side chains packed by a rotamer search, batched on the GPU.  ``sidechains.build`` builds the class the caller names; this module
CHOOSES the classes (th_pack_sidechains, csrc/pack_sidechains.hip) and then hands them to ``sidechains.build_arrays`` for the
atoms, the RMSD to the native and the clash counts.

    *** PARITY UNPINNED AGAINST SCWRL4 ***  The reference hands a sequence and a backbone to SCWRL4 (analyse_rotamers.py analyses 2
    and 3, ``pack_sidechains``), which is not available where this project is built.  The rule, written out in
    include/timed_hip.h, is this project's own:

    * the candidates of a residue are the 3^n_chi rotamer classes of its type, built at their bin centres (60 / 180 / -60 degrees)
      by the table of ``sidechains`` — not SCWRL4's backbone-dependent rotamer library;
    * the energy is an integer steric ladder — one unit of ``clash_weight`` for every ``ladder`` level that a pair of atoms of
      different residues is closer than, under the pair rules of the clash count — plus, optionally, a rotamer model's own
      probabilities as ``round(-1000 log2 p)`` (``prior_costs``).  There are no radii, no hydrogens, no hydrogen bonds, no
      solvation, no SCWRL4 energy;
    * the search is greedy: from the state in which every residue has its best candidate against the backbone alone, sweeps in
      residue order move a residue to its cheapest candidate when that is strictly cheaper.  It ends in a local minimum, not the
      global one, and is deterministic: two calls give the same bytes.

``clash_weight`` = 2000 says that one ladder level costs two bits of probability.  That is a choice, not a measurement: no real
model is available here to tune it against.  Without a prior, sterics alone is a weak packer (tests/golden/make_pack_golden.py
prints what it reaches on 1ubq); the prior-free mode is the model-independent baseline that analyse_rotamers.py --pack needs.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib, batching, pdbio, sidechains, structure
from ._lib import ptr

LADDER = (2.0, 2.5, 3.0, 3.5)             # Angstrom
CLASH_WEIGHT = 2000                        # one ladder level = two bits of probability: a choice, not a measurement
MAX_SWEEPS = 10
MAX_CANDIDATES = 81                        # TH_PACK_MAX_CANDIDATES: 3^4, ARG and LYS
MAX_COST = 1000000                         # TH_PACK_MAX_COST
MAX_STRUCT_RESIDUES = 4096                 # TH_PACK_MAX_STRUCT_RESIDUES
TH_PACK_OK, TH_PACK_TOO_LONG = 0, 1
BATCH_BYTES = batching.BATCH_BYTES
_UNIT_BYTES = 256                          # bytes per candidate of one call; a residue is counted as three candidates more


def candidate_counts(res_type) -> np.ndarray:
    """int64 [n]: 3^n_chi for a type with a side chain (1 for ALA), 0 for GLY and -1"""
    table = structure.rotamer_table()
    per_type = np.array([0 if res == "GLY" else 3 ** n_chi for res, n_chi, _, _ in table] + [0], dtype=np.int64)
    return per_type[np.asarray(res_type, dtype=np.int64)]


def prior_costs(matrix338, res_type) -> np.ndarray:
    """Rows of a 338-column rotamer probability matrix -> int32 [n, 81] costs for th_pack_sidechains: for a residue of type t with
    classes base .. base + n - 1, ``round(-1000 log2(p_k / sum of p over those classes))`` in float64, clipped to 1 000 000; p = 0
    maps to that cap; a row whose sum over the type's classes is 0 gives zeros (no preference), and so do GLY and type -1.
    Entries beyond the type's classes are 0."""
    matrix = np.asarray(matrix338, dtype=np.float64)
    res_type = np.asarray(res_type, dtype=np.int64).reshape(-1)
    table = structure.rotamer_table()
    n_classes = table[-1][2] + 3 ** table[-1][1]
    if matrix.ndim != 2 or matrix.shape != (res_type.size, n_classes):
        raise ValueError(f"the matrix needs the shape [{res_type.size}, {n_classes}]")
    if not (matrix >= 0).all():                                    # NaN fails too
        raise ValueError("probabilities are >= 0")
    if ((res_type < -1) | (res_type >= len(table))).any():
        raise ValueError("residue types run from -1 to 19")
    out = np.zeros((res_type.size, MAX_CANDIDATES), np.int32)
    for r, t in enumerate(res_type.tolist()):
        if t < 0 or table[t][0] == "GLY":
            continue
        base, n = table[t][2], 3 ** table[t][1]
        p = matrix[r, base:base + n]
        total = p.sum()
        if not total > 0 or not np.isfinite(total):
            continue
        with np.errstate(divide="ignore"):
            cost = np.rint(-1000.0 * np.log2(p / total))
        out[r, :n] = np.clip(np.where(p > 0, cost, MAX_COST), 0, MAX_COST).astype(np.int32)
    return out


@dataclass
class PackedArrays:
    cls: np.ndarray                        # [n_res] int16: the chosen class or -1
    cost_initial: np.ndarray               # [n_res] int64
    cost_final: np.ndarray                 # [n_res] int64
    energy_initial: np.ndarray             # [n_struct] int64
    energy_final: np.ndarray               # [n_struct] int64
    n_sweeps: np.ndarray                   # [n_struct] int32
    n_moves: np.ndarray                    # [n_struct] int32
    converged: np.ndarray                  # [n_struct] int32, 0 / 1
    status: np.ndarray                     # [n_struct] int32: TH_PACK_OK, TH_PACK_TOO_LONG


def pack_arrays(backbone, res_type, struct_offsets=None, chain_id=None, prior_cost=None, ladder: Sequence[float] = LADDER,
                clash_weight: int = CLASH_WEIGHT, max_sweeps: int = MAX_SWEEPS, device: int = 0, timing: Optional[dict] = None) -> PackedArrays:
    """One th_pack_sidechains call on flat arrays.  ``backbone`` [n_res, 3 or 4, 3], ``res_type`` [n_res] (-1..19, the type to
    build), ``struct_offsets`` [S + 1] (default: one structure), ``chain_id`` [n_res] or None, ``prior_cost`` int32 [n_res, 81] or
    None.  ``timing``: a dict whose ``kernel_ms`` grows by the device time of the kernels and whose ``pack_candidates_ms``,
    ``pack_backbone_ms`` and ``pack_search_ms`` grow by each kernel's."""
    backbone = np.ascontiguousarray(backbone, dtype=np.float64)
    res_type = np.ascontiguousarray(res_type, dtype=np.int8).reshape(-1)
    n_res = res_type.size
    if backbone.ndim != 3 or backbone.shape[0] != n_res or backbone.shape[1] not in (3, 4) or backbone.shape[2] != 3:
        raise ValueError(f"backbone needs the shape [{n_res}, 3 or 4, 3]")
    offsets = np.ascontiguousarray([0, n_res] if struct_offsets is None else struct_offsets, dtype=np.int64).reshape(-1)
    if offsets.size < 1:
        raise ValueError("struct_offsets needs at least one entry")
    if chain_id is not None:
        chain_id = np.ascontiguousarray(chain_id, dtype=np.int32).reshape(-1)
        if chain_id.size != n_res:
            raise ValueError(f"chain_id needs {n_res} entries")
    if prior_cost is not None:
        prior_cost = np.ascontiguousarray(prior_cost, dtype=np.int32)
        if prior_cost.shape != (n_res, MAX_CANDIDATES):
            raise ValueError(f"prior_cost needs the shape [{n_res}, {MAX_CANDIDATES}]")
    levels = np.ascontiguousarray(ladder, dtype=np.float64).reshape(-1)
    n_struct = offsets.size - 1
    cls = np.full(n_res, -1, np.int16)
    cost = np.zeros((2, n_res), np.int64)
    energy = np.zeros((2, n_struct), np.int64)
    search = np.zeros((n_struct, 4), np.int32)
    ms = (C.c_double * 3)()
    _lib.check(_lib.load().th_pack_sidechains(
        int(device), ptr(backbone), ptr(res_type), ptr(chain_id), ptr(offsets), n_struct, n_res, ptr(levels), levels.size, ptr(prior_cost),
        int(clash_weight), int(max_sweeps), sidechains.TH_SC_BACKBONE_O if backbone.shape[1] == 4 else 0, ptr(cls), ptr(cost[0]), ptr(cost[1]),
        ptr(energy[0]), ptr(energy[1]), ptr(search), C.cast(ms, C.c_void_p) if timing is not None else None))
    if timing is not None:
        timing["kernel_ms"] = timing.get("kernel_ms", 0.0) + sum(ms)
        for name, value in zip(("pack_candidates_ms", "pack_backbone_ms", "pack_search_ms"), ms):
            timing[name] = timing.get(name, 0.0) + value
    return PackedArrays(cls, cost[0].copy(), cost[1].copy(), energy[0].copy(), energy[1].copy(), search[:, 0].copy(), search[:, 1].copy(),
                        search[:, 2].copy(), search[:, 3].copy())


@dataclass
class PackedSidechains:
    cls: np.ndarray                        # [n] int16: the packed class or -1
    chi: np.ndarray                        # [n, 4] float64: the centres of the class's bins
    res_type: np.ndarray                   # [n] int8: the type that was packed
    cost_initial: np.ndarray               # [n] int64
    cost_final: np.ndarray                 # [n] int64
    energy_initial: int
    energy_final: int
    n_sweeps: int
    n_moves: int
    converged: bool
    status: int
    unmatched_rows: int                    # rows of the dataset map that name no residue of the structure
    built: sidechains.BuiltSidechains      # th_build_sidechains on the packed classes

    @property
    def residues(self) -> List[pdbio.Residue]:
        return self.built.residues


def rows_for_residues(map_rows, labels, layouts) -> List[Tuple[np.ndarray, int]]:
    """per structure (int64 [n] matrix row of each residue or -1, rows of the map without a residue): map row k = (pdb, chain,
    residue number, label) belongs to the first residue of that chain and number in the structure whose file name starts with the
    pdb code — the rule of ``structure.labels_for_map``"""
    if any(len(row) < 4 for row in map_rows):
        raise ValueError("the dataset map must be the csv map with one (pdb, chain, residue number, label) row per matrix row: "
                         "residues are paired by chain and number")
    per_code: dict = {}
    for k, row in enumerate(map_rows):
        per_code.setdefault(str(row[0])[:4].lower(), []).append((str(row[1]).strip(), str(row[2]).strip(), k))
    out = []
    for label, layout in zip(labels, layouts):
        rows = np.full(len(layout.residues), -1, np.int64)
        unmatched = 0
        by_key: dict = {}
        for r, res in enumerate(layout.residues):
            by_key.setdefault((res.chain, res.number), r)
        for chain, number, k in per_code.get(pdbio.stem_of(label)[:4].lower(), []):
            if (chain, number) in by_key:
                rows[by_key[(chain, number)]] = k
            else:
                unmatched += 1
        out.append((rows, unmatched))
    return out


def cut_batches(sizes: Sequence[int], budget_bytes: int = BATCH_BYTES) -> List[Tuple[int, int]]:
    """[lo, hi) runs of consecutive structures whose candidates (``sizes``: candidates + three per residue) fit ``budget_bytes``"""
    return batching.cut_batches(sizes, budget_bytes, _UNIT_BYTES)


def pack(structures: Sequence[Union[pdbio.Model, structure.RotamerLayout, str, os.PathLike]], sequence: str = "native", matrix=None,
         dataset_map=None, prior: Optional[str] = None, types=None, ladder: Sequence[float] = LADDER, clash_weight: int = CLASH_WEIGHT,
         max_sweeps: int = MAX_SWEEPS, clash_distance: float = sidechains.CLASH_DISTANCE, device: int = 0, labels: Optional[Sequence[str]] = None,
         budget_bytes: int = BATCH_BYTES, stats: Optional[dict] = None) -> List[PackedSidechains]:
    """Pack the side chains of every structure (``pdbio.Model`` objects, ``RotamerLayout`` objects or paths) on its native backbone.

    ``sequence``: ``"native"`` packs the residue types of the structure; ``"predicted"`` packs, for every residue, the type of the
    arg-max class (the first maximum) of its matrix row, as build_sidechains.py does; a residue without a row stays unbuilt.
    ``matrix`` [rows, 338] with ``dataset_map`` (rows (pdb, chain, residue number, label), one per matrix row) pairs rows with
    residues by chain and residue number; ``labels`` are the structures' file names (default: the paths given).
    ``types``: per structure an array of residue types (-1..19) to pack instead of what ``sequence`` names.
    ``prior``: ``"matrix"`` (the default with a matrix) adds ``prior_costs`` of the rows, renormalised over the classes of the type
    that is packed; ``"none"`` (the default without) packs by sterics alone.
    One th_pack_sidechains call and one th_build_sidechains call per batch, cut by ``budget_bytes`` over the candidates; ``stats``
    receives ``submissions``, ``kernel_ms`` and the time of each kernel."""
    if sequence not in ("native", "predicted"):
        raise ValueError(f"sequence is \"native\" or \"predicted\", not {sequence!r}")
    prior = prior or ("matrix" if matrix is not None else "none")
    if prior not in ("matrix", "none"):
        raise ValueError(f"prior is \"matrix\" or \"none\", not {prior!r}")
    if matrix is None and (prior == "matrix" or sequence == "predicted"):
        raise ValueError("a predicted sequence and a matrix prior need a matrix and its dataset map")
    natives = [s if isinstance(s, structure.RotamerLayout) else structure.rotamer_layout(structure.first_model(s)) for s in structures]
    table = structure.rotamer_table()
    bases = np.array([base for _, _, base, _ in table], dtype=np.int64)
    paired = [(None, 0)] * len(natives)
    if matrix is not None:
        matrix = np.asarray(matrix, dtype=np.float64)
        if dataset_map is None or len(dataset_map) != len(matrix):
            raise ValueError(f"the dataset map needs one row per matrix row ({len(matrix)})")
        if labels is None:
            labels = [str(s) for s in structures]
        if len(labels) != len(natives):
            raise ValueError(f"labels need one entry per structure ({len(natives)})")
        paired = rows_for_residues(dataset_map, labels, natives)
    if types is not None and len(types) != len(natives):
        raise ValueError(f"types need one entry per structure ({len(natives)})")
    layouts = []
    for s, (native, (rows, unmatched)) in enumerate(zip(natives, paired)):
        backbone, chain_id = sidechains.backbone_of(native.residues)
        res_type = np.ascontiguousarray(native.res_type, dtype=np.int8)
        have = None if rows is None else rows >= 0
        if sequence == "predicted":
            chosen = np.argmax(matrix[np.maximum(rows, 0)], axis=1) if len(rows) else np.zeros(0, np.int64)
            res_type = np.where(have, np.searchsorted(bases, chosen, side="right") - 1, -1).astype(np.int8)
        if types is not None:
            res_type = np.ascontiguousarray(types[s], dtype=np.int8).reshape(-1)
            if res_type.size != len(native.residues):
                raise ValueError(f"structure {s} has {len(native.residues)} residues and {res_type.size} types")
        cost = None
        if prior == "matrix":
            cost = prior_costs(np.where(have[:, None], matrix[np.maximum(rows, 0)], 0.0), res_type)
        layouts.append((native, backbone, chain_id, res_type, cost, unmatched))
    out: List[PackedSidechains] = []

    def submit(part, timing):
        res_lo = np.zeros(len(part) + 1, np.int64)
        np.cumsum([len(p[3]) for p in part], out=res_lo[1:])
        backbone, chain_id = np.concatenate([p[1] for p in part]), np.concatenate([p[2] for p in part])
        res_type = np.concatenate([p[3] for p in part])
        cost = np.concatenate([p[4] for p in part]) if prior == "matrix" else None
        got = pack_arrays(backbone, res_type, res_lo, chain_id, cost, ladder, clash_weight, max_sweeps, device, timing)
        _, chi = sidechains.class_centres(got.cls)                     # a residue without a class keeps its packed type and stays unbuilt
        built = sidechains.build_layouts([sidechains.SidechainLayout(p[0], p[1], p[2], p[3], chi[lo:hi], got.cls[lo:hi].copy())
                                          for p, lo, hi in zip(part, res_lo[:-1], res_lo[1:])], clash_distance, device, 1 << 62, None)
        for k, p in enumerate(part):
            lo, hi = res_lo[k], res_lo[k + 1]
            out.append(PackedSidechains(got.cls[lo:hi].copy(), chi[lo:hi].copy(), p[3], got.cost_initial[lo:hi].copy(), got.cost_final[lo:hi].copy(),
                                        int(got.energy_initial[k]), int(got.energy_final[k]), int(got.n_sweeps[k]), int(got.n_moves[k]),
                                        bool(got.converged[k]), int(got.status[k]), p[5], built[k]))
    sizes = [int(candidate_counts(p[3]).sum()) + 3 * len(p[3]) for p in layouts]
    timing_keys = ("pack_candidates_ms", "pack_backbone_ms", "pack_search_ms")
    runs = cut_batches(sizes, budget_bytes)
    timing = {} if stats is not None else None
    for lo, hi in runs:
        submit(layouts[lo:hi], timing)
    if stats is not None:
        stats["submissions"] = stats.get("submissions", 0) + len(runs)
        for key in ("kernel_ms",) + timing_keys:
            stats[key] = stats.get(key, 0.0) + timing.get(key, 0.0)
    return out
