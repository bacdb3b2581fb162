"""Superposition of models on their native, batched on the GPU: RMSD, the GDT fractions and the per-residue deviation of every
(reference, model) pair — the reference's ``calculate_RMSD_and_gdt`` (scripts/analyse_af2.py), which loads each pair into PyMOL,
selects ``name CA``, calls ``cmd.align`` and averages the fractions of aligned pairs within 1, 2, 4 and 8 Angstrom — through
th_superpose (csrc/superpose.hip): one wavefront per pair, every pair of a batch and every refinement cycle in one launch.

    *** PARITY UNPINNED AGAINST PYMOL ***  PyMOL is not available where this project is built.  The rule is this project's reading of
    the documented behaviour of ``cmd.align`` (``cycles`` 5, ``cutoff`` 2.0) on atoms that are ALREADY PAIRED, written out in
    include/timed_hip.h: a least-squares fit with the proper rotation (Horn's quaternion), then up to ``cycles`` rounds that drop the
    kept positions further than ``cutoff`` x RMS and fit again.  No sequence alignment is made: the reference itself asserts that
    native and model are equally long, they are designs on one backbone.

    * the first model of a file; ATOM records only (non-hetero residues); of alternate locations the first (``pdbio``);
    * one position per residue that has the atom (``atom="CA"``), chains in file order;
    * ``pair_by="position"``: positions are paired in file order; lists of different length are that pair's ``error``;
    * ``pair_by="number"``: positions are paired on (chain, residue number with insertion code), in the reference's order; what
      either side has alone is counted in ``unpaired_reference`` / ``unpaired_model``.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib, batching, pdbio, structure
from ._lib import ptr

PAIR_BY = ("position", "number")
GDT_CUTOFFS = (1.0, 2.0, 4.0, 8.0)
_POSITION_BYTES = 2 * 3 * 8 + 8 + 1        # both coordinate lists, distance, kept byte
_CHARGED_BYTES = 2 * structure._ATOM_BYTES  # what a position is charged against the budget: two atoms, more than it takes


class Superposed(NamedTuple):
    """What one th_superpose call returns."""
    dist: np.ndarray                   # [total] float64: d_i under the final fit, NaN at an invalid position
    kept: np.ndarray                   # [total] uint8
    rmsd: np.ndarray                   # [pairs, 3] float64: rmsd_kept, rmsd_all, rmsd_fit_all
    counts: np.ndarray                 # [pairs, 7] int32: n_valid, n_kept, cycles_run, within 1, 2, 4, 8 Angstrom
    transform: Optional[np.ndarray]    # [pairs, 3, 4] float64 [R | t], moved = R mob + t; None unless asked for


def superpose_arrays(ref_xyz, mob_xyz, offsets, cycles: int = 5, cutoff: float = 2.0, device: int = 0, transform: bool = False,
                     timing: Optional[dict] = None) -> Superposed:
    """One th_superpose call.  ``ref_xyz`` / ``mob_xyz`` [total, 3] float64, ``offsets`` [pairs + 1].  ``timing``: a dict whose
    ``kernel_ms`` grows by the device time of the kernel."""
    ref_xyz = np.ascontiguousarray(ref_xyz, dtype=np.float64).reshape(-1, 3)
    mob_xyz = np.ascontiguousarray(mob_xyz, dtype=np.float64).reshape(-1, 3)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    if offsets.size < 1:
        raise ValueError("offsets needs at least one entry")
    if ref_xyz.shape != mob_xyz.shape:
        raise ValueError(f"ref_xyz has {ref_xyz.shape[0]} positions, mob_xyz {mob_xyz.shape[0]}")
    total, n_pairs = ref_xyz.shape[0], offsets.size - 1
    dist = np.empty(total, np.float64)
    kept = np.empty(total, np.uint8)
    rmsd = np.empty((n_pairs, 3), np.float64)
    counts = np.empty((n_pairs, 7), np.int32)
    moves = np.empty((n_pairs, 3, 4), np.float64) if transform else None
    ms = C.c_double(0.0)
    _lib.check(_lib.load().th_superpose(int(device), ptr(ref_xyz), ptr(mob_xyz), total, ptr(offsets), n_pairs, int(cycles), float(cutoff),
                                        ptr(dist), ptr(kept), ptr(rmsd), ptr(counts), ptr(moves), C.byref(ms) if timing is not None else None))
    if timing is not None:
        timing["kernel_ms"] = timing.get("kernel_ms", 0.0) + ms.value
    return Superposed(dist, kept, rmsd, counts, moves)


@dataclass
class AtomLayout:
    """One structure as superpose() pairs it: one position per residue that has the atom."""
    xyz: np.ndarray                    # [n, 3] float64
    residues: List[pdbio.Residue]      # the residue of each position


def atom_layout(model: pdbio.Model, atom: str = "CA") -> AtomLayout:
    """The ``atom`` of every non-hetero residue that has one, chains in file order (a chain that comes back later in the file
    continues its entry)."""
    chains: Dict[str, List[pdbio.Residue]] = {}
    for r in model.residues:
        if not r.hetero and atom in r.atoms:
            chains.setdefault(r.chain, []).append(r)
    residues = [r for members in chains.values() for r in members]
    return AtomLayout(np.array([r.atoms[atom] for r in residues], dtype=np.float64).reshape(-1, 3), residues)


@dataclass
class PairResult:
    error: Optional[str]               # why the pair was not scored (every figure below is then NaN / 0 / empty)
    n_valid: int
    n_kept: int
    cycles_run: int
    rmsd_kept: float                   # the number cmd.align returns
    rmsd_all: float
    rmsd_fit_all: float                # the conventional RMSD: one fit over every valid position
    gdt: Tuple[float, float, float, float]     # fractions of the valid positions within 1, 2, 4, 8 Angstrom under the final fit
    mean_gdt: float
    sequence_identity: float           # fraction of paired positions whose residue names agree (the reference's seq_accuracy)
    dist: np.ndarray                   # [paired positions] float64
    kept: np.ndarray                   # [paired positions] uint8
    residues: List[pdbio.Residue]      # the REFERENCE's residue of each paired position
    unpaired_reference: int
    unpaired_model: int
    transform: Optional[np.ndarray] = None     # [3, 4], when asked for


def _failed(error: str, unpaired_reference: int = 0, unpaired_model: int = 0) -> PairResult:
    nan = float("nan")
    return PairResult(error, 0, 0, 0, nan, nan, nan, (nan, nan, nan, nan), nan, nan, np.zeros(0, np.float64), np.zeros(0, np.uint8), [],
                      unpaired_reference, unpaired_model)


def gdt_fractions(counts) -> Tuple[Tuple[float, float, float, float], float]:
    """The four fractions and their mean (the reference's ``mean_gdt``) from one row of th_superpose's counts."""
    n_valid = int(counts[0])
    if n_valid == 0:
        nan = float("nan")
        return (nan, nan, nan, nan), nan
    gdt = tuple(int(c) / n_valid for c in counts[3:7])
    return gdt, float(np.mean(gdt))


def pair_positions(reference: AtomLayout, model: AtomLayout, pair_by: str = "position"):
    """-> (indices into the reference, indices into the model, error or None)"""
    if pair_by == "position":
        if len(reference.residues) != len(model.residues):
            return None, None, f"length mismatch: reference has {len(reference.residues)} positions, model {len(model.residues)}"
        index = np.arange(len(reference.residues))
        return index, index, None
    if pair_by == "number":
        where = {}
        for k, r in enumerate(model.residues):
            where.setdefault((r.chain, r.number), k)
        ours, theirs = [], []
        for k, r in enumerate(reference.residues):
            j = where.pop((r.chain, r.number), None)
            if j is not None:
                ours.append(k)
                theirs.append(j)
        return np.array(ours, dtype=np.int64), np.array(theirs, dtype=np.int64), None
    raise ValueError(f"pair_by {pair_by!r} not in {PAIR_BY}")


def _load_layouts(items, atom: str, workers: int) -> List[Optional[Union[AtomLayout, str]]]:
    """Every distinct file is read once (a native shared by a thousand models too), on host threads; a file that cannot be read
    becomes the error text of the pairs that name it."""
    paths = list(dict.fromkeys(os.fspath(item) for item in items if not isinstance(item, (AtomLayout, pdbio.Model))))

    def parse(path):
        try:
            return atom_layout(structure.first_model(path), atom)
        except (OSError, EOFError, ValueError) as e:
            return f"{path}: {e}"
    paths = dict(zip(paths, batching.parse_each(parse, paths, workers)))
    models, out = {}, []
    for item in items:
        if isinstance(item, AtomLayout):
            out.append(item)
        elif isinstance(item, pdbio.Model):
            if id(item) not in models:
                models[id(item)] = atom_layout(item, atom)
            out.append(models[id(item)])
        else:
            out.append(paths[os.fspath(item)])
    return out


@dataclass
class Prepared:
    """What prepare() returns, and what superpose() and lddt.lddt() take in place of raw pairs."""
    pairs: list                        # per pair (reference layout, model layout, indices into each), or the text of its error
    files: int                         # distinct files read
    atom: str
    counted: list = field(default_factory=list)        # the stats dicts that hold ``files`` already


def prepare(pairs: Sequence[Tuple], pair_by: str = "position", atom: str = "CA", workers: int = 8) -> Prepared:
    """Read every distinct file of the ``(reference, model)`` pairs once and pair the positions of each pair once, for any number
    of scorers: ``superpose(prepared, ...)`` and ``lddt.lddt(prepared, ...)`` then read and pair nothing (their ``pair_by``,
    ``atom`` and ``workers`` are not looked at), and of the scorers that share one ``stats`` dict the first adds ``files_parsed``.
    What prepare() returned comes back as it is."""
    if isinstance(pairs, Prepared):
        return pairs
    if pair_by not in PAIR_BY:
        raise ValueError(f"pair_by {pair_by!r} not in {PAIR_BY}")
    sides = [side for pair in pairs for side in pair[:2]]
    flat = _load_layouts(sides, atom, workers)
    out = []
    for ref, mod in zip(flat[0::2], flat[1::2]):
        broken = [side for side in (ref, mod) if isinstance(side, str)]
        if broken:
            out.append("; ".join(broken))
            continue
        ours, theirs, error = pair_positions(ref, mod, pair_by)
        out.append(error or (ref, mod, ours, theirs))
    return Prepared(out, len({os.fspath(s) for s in sides if not isinstance(s, (AtomLayout, pdbio.Model))}), atom)


def score_pairs(prepared: Prepared, budget_bytes: int, stats: Optional[dict], position_bytes: int, arrays: Callable, result: Callable,
                failed: Callable, cost: Optional[Callable] = None, whole_pairs: bool = False) -> list:
    """The driver superpose(), lddt.lddt() and tmscore.tmscore() share: the pairs that can be scored go in batches of
    ``position_bytes`` per position under ``budget_bytes``, one ``arrays(ref_xyz, mob_xyz, offsets, timing)`` call each; a pair's
    result is ``result(got, j, a, b, ref, mod, ours, theirs)`` — pair j of the call, positions [a, b) of its flat arrays — or
    ``failed(error text)``.  ``stats`` receives ``submissions``, ``kernel_ms`` and ``files_parsed``.  ``cost(ref, mod, ours,
    theirs)``, when given, is what a pair is charged in units of ``position_bytes`` instead of its number of positions;
    ``whole_pairs``: ``arrays`` receives a fifth argument, the ``(ref, mod, ours, theirs)`` of the pairs of its call."""
    results = [failed(item) if isinstance(item, str) else None for item in prepared.pairs]
    ready = [(k,) + item for k, item in enumerate(prepared.pairs) if not isinstance(item, str)]

    def submit(part, timing):
        offsets = np.zeros(len(part) + 1, np.int64)
        np.cumsum([len(item[3]) for item in part], out=offsets[1:])
        ref_xyz = np.concatenate([ref.xyz[ours] for _, ref, _, ours, _ in part])
        mob_xyz = np.concatenate([mod.xyz[theirs] for _, _, mod, _, theirs in part])
        got = arrays(ref_xyz, mob_xyz, offsets, timing, [item[1:] for item in part]) if whole_pairs else arrays(ref_xyz, mob_xyz, offsets, timing)
        for j, (k, ref, mod, ours, theirs) in enumerate(part):
            results[k] = result(got, j, int(offsets[j]), int(offsets[j + 1]), ref, mod, ours, theirs)
    batching.run_batches(ready, [cost(*item[1:]) if cost else len(item[3]) for item in ready], budget_bytes, position_bytes, submit, stats)
    if stats is not None and not any(seen is stats for seen in prepared.counted):
        prepared.counted.append(stats)
        stats["files_parsed"] = stats.get("files_parsed", 0) + prepared.files
    return results


def superpose(pairs: Sequence[Tuple], pair_by: str = "position", atom: str = "CA", cycles: int = 5, cutoff: float = 2.0, device: int = 0,
              transform: bool = False, workers: int = 8, budget_bytes: int = structure.BATCH_BYTES, stats: Optional[dict] = None) -> List[PairResult]:
    """Every ``(reference, model)`` pair — paths of PDB files (plain or gzipped), ``pdbio.Model`` objects or ``AtomLayout`` objects —
    superposed under the rule of the module docstring.  One GPU call per batch; batches are cut by ``structure.cut_batches`` under
    ``budget_bytes`` (a position counts as two atoms: it has two coordinate lists).  A pair that cannot be scored carries its
    ``error`` and does not stop the others.  ``stats`` receives ``submissions``, ``kernel_ms`` and ``files_parsed``.  ``pairs`` may
    be what ``prepare`` returned."""
    def result(got, j, a, b, ref, mod, ours, theirs):
        counts = got.counts[j]
        gdt, mean_gdt = gdt_fractions(counts)
        same = sum(ref.residues[i].name == mod.residues[t].name for i, t in zip(ours, theirs))
        return PairResult(None, int(counts[0]), int(counts[1]), int(counts[2]), float(got.rmsd[j, 0]), float(got.rmsd[j, 1]),
                          float(got.rmsd[j, 2]), gdt, mean_gdt, same / len(ours) if len(ours) else float("nan"), got.dist[a:b].copy(),
                          got.kept[a:b].copy(), [ref.residues[i] for i in ours], len(ref.residues) - len(ours),
                          len(mod.residues) - len(theirs), got.transform[j].copy() if transform else None)
    return score_pairs(prepare(pairs, pair_by, atom, workers), budget_bytes, stats, _CHARGED_BYTES,
                       lambda ref_xyz, mob_xyz, offsets, timing: superpose_arrays(ref_xyz, mob_xyz, offsets, cycles, cutoff, device, transform, timing),
                       result, _failed)
