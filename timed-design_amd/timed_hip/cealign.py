"""Structural alignment of models of ANY length on their native, batched on the GPU: the sequence-independent alignment by
combinatorial extension (CE, Shindyalov & Bourne 1998) that the reference gets one pair at a time from PyMOL's ``cmd.cealign`` on the
CA atoms (scripts/analyse_all_properties.py ``_calculate_RMSD``, scripts/analyse_cherrypicked_samples_af2.py) — through th_cealign
(csrc/cealign.hip): every fragment pair of every structure pair is one wavefront.  The two chains need not be equally long nor
numbered alike; the alignment that comes out is a pairing, and ``prepare_aligned`` hands it to ``superpose.superpose``,
``lddt.lddt`` and ``tmscore.tmscore`` unchanged.

    *** PARITY UNPINNED AGAINST PYMOL ***  PyMOL is not available where this project is built.  The rule is this project's reading of
    the published CE algorithm with cealign's documented defaults, written out in include/timed_hip.h: fragments of 8 positions;
    a fragment pair is similar when the mean difference of its 21 inner distances is below ``d0`` (3.0); from every similar pair a
    path is extended greedily over ``2 gap_max + 1`` (61) gapped candidates per step, by the smallest mean inter-fragment distance,
    while that and the path's score stay below ``d1`` (4.0); the 20 longest (then best-scoring) paths are fitted with the fit of
    ``superpose`` and the one of smallest RMSD wins.

    * structures are read exactly as ``timed_hip.superpose`` reads them: the first model, one position per residue that has the atom;
    * a structure of more than ``MAX_POSITIONS`` (2048) positions carries that as its pair's ``error``;
    * no fragment pair similar enough is a RESULT, not an error: ``n_afps`` 0, NaN figures, nothing aligned;
    * MIRROR IMAGES: CE compares distances and does not see a mirror image; the proper rotation then refuses to fit it (the mirrored
      1ubq aligns 64 positions at 9.55 Angstrom).
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _lib, batching, pdbio, structure
from ._lib import ptr
from .superpose import AtomLayout, Prepared, _load_layouts

D0, D1, GAP_MAX = 3.0, 4.0, 30
MAX_POSITIONS = 2048               # TH_CE_MAX_POSITIONS
WINDOW = 8                         # TH_CE_WINDOW
KEEP = 20                          # TH_CE_KEEP
_WINDOW_PAIR_BYTES = 8 + 4 + 8     # S, and a start's record: the length and the score of its path
_WINDOW_BYTES = 21 * 8             # the inner distances of one window start
_POSITION_BYTES = 3 * 8 + 4 + 4    # compacted coordinates, the index map, and (reference side) the aligned index


class CeTables(NamedTuple):
    """What one th_cealign call returns."""
    align: np.ndarray                  # [ref_total] int32: the model position, local to the pair, aligned to this reference position; -1 if none
    scores: np.ndarray                 # [pairs, 2] float64: rmsd over the aligned positions, path score
    counts: np.ndarray                 # [pairs, 6] int64: mA, mB, n_starts, n_afps, n_aligned, n_candidates
    transform: Optional[np.ndarray]    # [pairs, 3, 4] float64 [R | t], moved = R mob + t; None unless asked for


def cealign_arrays(ref_xyz, ref_offsets, mob_xyz, mob_offsets, d0: float = D0, d1: float = D1, gap_max: int = GAP_MAX, device: int = 0,
                   transform: bool = False, timing: Optional[dict] = None) -> CeTables:
    """One th_cealign call.  ``ref_xyz`` [ref_total, 3] and ``mob_xyz`` [mob_total, 3] float64, each with its own ``offsets``
    [pairs + 1].  ``timing``: a dict whose ``kernel_ms`` grows by the device time of the kernels."""
    ref_xyz = np.ascontiguousarray(ref_xyz, dtype=np.float64).reshape(-1, 3)
    mob_xyz = np.ascontiguousarray(mob_xyz, dtype=np.float64).reshape(-1, 3)
    ref_offsets = np.ascontiguousarray(ref_offsets, dtype=np.int64).reshape(-1)
    mob_offsets = np.ascontiguousarray(mob_offsets, dtype=np.int64).reshape(-1)
    if ref_offsets.size < 1 or ref_offsets.size != mob_offsets.size:
        raise ValueError(f"ref_offsets has {ref_offsets.size} entries, mob_offsets {mob_offsets.size}: both need pairs + 1")
    n_pairs = ref_offsets.size - 1
    align = np.empty(ref_xyz.shape[0], np.int32)
    scores = np.empty((n_pairs, 2), np.float64)
    counts = np.empty((n_pairs, 6), np.int64)
    moves = np.empty((n_pairs, 3, 4), np.float64) if transform else None
    ms = C.c_double(0.0)
    _lib.check(_lib.load().th_cealign(int(device), ptr(ref_xyz), ref_xyz.shape[0], ptr(ref_offsets), ptr(mob_xyz), mob_xyz.shape[0], ptr(mob_offsets),
                                      n_pairs, float(d0), float(d1), int(gap_max), ptr(align), ptr(scores), ptr(counts), ptr(moves),
                                      C.byref(ms) if timing is not None else None))
    if timing is not None:
        timing["kernel_ms"] = timing.get("kernel_ms", 0.0) + ms.value
    return CeTables(align, scores, counts, moves)


@dataclass
class CeResult:
    error: Optional[str]               # why the pair was not aligned (every figure below is then NaN / 0 / empty)
    n_ref: int                         # valid positions of the reference
    n_model: int
    n_starts: int
    n_afps: int
    n_aligned: int
    n_candidates: int
    rmsd: float                        # over the aligned positions under the winning fit: the number cmd.cealign returns
    path_score: float
    reference_index: np.ndarray        # [n_aligned] int64: positions of the reference's layout, ascending
    model_index: np.ndarray            # [n_aligned] int64: the model position aligned to each
    reference: Optional[AtomLayout] = None
    model: Optional[AtomLayout] = None
    transform: Optional[np.ndarray] = None     # [3, 4], when asked for


def _failed(error: str) -> CeResult:
    nan = float("nan")
    return CeResult(error, 0, 0, 0, 0, 0, 0, nan, nan, np.zeros(0, np.int64), np.zeros(0, np.int64))


def pair_bytes(n_ref: int, n_model: int) -> int:
    """What a pair takes of the byte budget: its S matrix and per-start records, its window rows and its positions."""
    ra, rb = max(int(n_ref) - WINDOW + 1, 0), max(int(n_model) - WINDOW + 1, 0)
    if ra == 0 or rb == 0:
        ra = rb = 0
    return ra * rb * _WINDOW_PAIR_BYTES + (ra + rb) * _WINDOW_BYTES + (int(n_ref) + int(n_model)) * _POSITION_BYTES


def cealign(pairs: Sequence[Tuple], atom: str = "CA", d0: float = D0, d1: float = D1, gap_max: int = GAP_MAX, device: int = 0,
            transform: bool = False, workers: int = 8, budget_bytes: int = structure.BATCH_BYTES, stats: Optional[dict] = None) -> List[CeResult]:
    """Every ``(reference, model)`` pair — paths of PDB files (plain or gzipped), ``pdbio.Model`` objects or ``AtomLayout`` objects, as
    for ``superpose.superpose`` — aligned under the rule of the module docstring.  Every distinct file is read once; one GPU call per
    batch; a pair is charged ``pair_bytes`` against ``budget_bytes`` (20 bytes per fragment pair: 95 KB for two chains of 76, 1.7 MB
    for two of 300).  A pair that cannot be aligned — a structure of more than 2048 positions among them — carries its ``error`` and
    does not stop the others.  ``stats`` receives ``submissions``, ``kernel_ms`` and ``files_parsed``."""
    if not (float(d0) > 0 and float(d0) < float("inf")) or not (float(d1) > 0 and float(d1) < float("inf")):
        raise ValueError(f"d0 = {d0} and d1 = {d1} must be positive finite numbers")
    if not 0 <= int(gap_max) <= 31:
        raise ValueError(f"gap_max = {gap_max} is outside 0 .. 31")
    sides = [side for pair in pairs for side in pair[:2]]
    flat = _load_layouts(sides, atom, workers)
    results: List[Optional[CeResult]] = []
    ready = []
    for k, (ref, mod) in enumerate(zip(flat[0::2], flat[1::2])):
        broken = [side for side in (ref, mod) if isinstance(side, str)]
        longest = 0 if broken else max(len(ref.residues), len(mod.residues))
        if broken:
            results.append(_failed("; ".join(broken)))
        elif longest > MAX_POSITIONS:
            results.append(_failed(f"{longest} positions in one structure: th_cealign takes {MAX_POSITIONS} at most"))
        else:
            results.append(None)
            ready.append((k, ref, mod))

    def submit(part, timing):
        ref_offsets = np.zeros(len(part) + 1, np.int64)
        mob_offsets = np.zeros(len(part) + 1, np.int64)
        np.cumsum([len(ref.xyz) for _, ref, _ in part], out=ref_offsets[1:])
        np.cumsum([len(mod.xyz) for _, _, mod in part], out=mob_offsets[1:])
        got = cealign_arrays(np.concatenate([ref.xyz.reshape(-1, 3) for _, ref, _ in part]), ref_offsets,
                             np.concatenate([mod.xyz.reshape(-1, 3) for _, _, mod in part]), mob_offsets, d0, d1, gap_max, device, transform, timing)
        for j, (k, ref, mod) in enumerate(part):
            partner = got.align[int(ref_offsets[j]):int(ref_offsets[j + 1])]
            ours = np.nonzero(partner >= 0)[0].astype(np.int64)
            counts = [int(c) for c in got.counts[j]]
            results[k] = CeResult(None, *counts, float(got.scores[j, 0]), float(got.scores[j, 1]), ours, partner[ours].astype(np.int64), ref, mod,
                                  got.transform[j].copy() if transform else None)
    sizes = [pair_bytes(int(np.isfinite(ref.xyz).all(axis=1).sum()), int(np.isfinite(mod.xyz).all(axis=1).sum())) for _, ref, mod in ready]
    batching.run_batches(ready, sizes, budget_bytes, 1, submit, stats)
    if stats is not None:
        stats["files_parsed"] = stats.get("files_parsed", 0) + len({os.fspath(s) for s in sides if not isinstance(s, (AtomLayout, pdbio.Model))})
    return results


def prepare_aligned(pairs: Sequence[Tuple], atom: str = "CA", d0: float = D0, d1: float = D1, gap_max: int = GAP_MAX, device: int = 0,
                    workers: int = 8, budget_bytes: int = structure.BATCH_BYTES, stats: Optional[dict] = None,
                    results: Optional[List[CeResult]] = None) -> Prepared:
    """A ``superpose.Prepared`` whose index pairs are the CE alignment of every pair: ``superpose.superpose``, ``lddt.lddt`` and
    ``tmscore.tmscore`` then score the aligned positions unchanged (what either side has alone counts as unpaired).  A pair without
    an alignment is paired at no position.  ``results``: what ``cealign`` already returned for the same pairs — nothing is aligned twice."""
    if results is None:
        results = cealign(pairs, atom, d0, d1, gap_max, device, False, workers, budget_bytes, stats)
    sides = [side for pair in pairs for side in pair[:2]]
    out = [res.error if res.error else (res.reference, res.model, res.reference_index, res.model_index) for res in results]
    prepared = Prepared(out, len({os.fspath(s) for s in sides if not isinstance(s, (AtomLayout, pdbio.Model))}), atom)
    if stats is not None:
        prepared.counted.append(stats)                                 # cealign() counted the files already
    return prepared
