"""TM-score of models against their native, batched on the GPU: the template-modelling score (Zhang & Skolnick 2004) of every
(reference, model) pair through th_tmscore (csrc/tmscore.hip) — the "scTM against the native" of a design pipeline's
self-consistency check.  The score is the MAXIMUM over superpositions of ``sum_i 1 / (1 + (d_i / d0)^2) / L``; the superposition
that attains it is in general not the least-squares fit of ``timed_hip.superpose``, so it is searched for: every seed of every pair
is one wavefront.

    *** PARITY UNPINNED AGAINST THE TM-score PROGRAM ***  Zhang & Skolnick's TMscore is not available where this project is built.
    The rule is this project's reading of the published definition and search, written out in include/timed_hip.h: ``d0 = max(0.5,
    1.24 cbrt(L - 15) - 1.8)``; seeds are the windows of length m, m div 2, ... >= 4 at every start; each seed is fitted (the fit of
    ``superpose``), scored over all positions, and re-fitted over the positions closer than ``d_search -/+ 1`` Angstrom until the set
    stops changing or ``rounds`` are used up; the best score of any round of any seed is the pair's.  No sequence alignment is made
    (that is TM-align, not TM-score).

    * structures are read and positions are paired exactly as ``timed_hip.superpose`` does (``pair_by="position"`` or ``"number"``);
    * ``norm_length`` is the number of residues of the REFERENCE that have the atom: under ``pair_by="number"`` the residues that the
      model lacks therefore cost score;
    * a pair of more than ``MAX_POSITIONS`` (4096) positions carries that as its ``error``: the kernel keeps a seed's set as one
      64-bit mask per lane;
    * MIRROR IMAGES: the rotation is proper, so a mirror image scores low (0.31 for the mirrored 1ubq, which lDDT scores 1.0).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _lib, pdbio, structure
from ._lib import ptr
from .superpose import Prepared, prepare, score_pairs

ROUNDS = 20
MAX_POSITIONS = 4096               # TH_TM_MAX_POSITIONS
_POSITION_BYTES = 2 * 3 * 8 + 4 + 8        # both compacted coordinate lists, the index map and the distance
_SEED_BYTES = 8 + 4                        # a seed's best score and its number of fits


class TmTables(NamedTuple):
    """What one th_tmscore call returns."""
    tm: np.ndarray                     # [pairs, 2] float64: tm, d0
    counts: np.ndarray                 # [pairs, 4] int64: n_valid, L, n_seeds, n_fits
    dist: Optional[np.ndarray]         # [total] float64: d_i under the best superposition, NaN at an invalid position; None unless asked for
    transform: Optional[np.ndarray]    # [pairs, 3, 4] float64 [R | t] of the best superposition; None unless asked for


def d0(norm_length: int) -> float:
    """th_tm_d0: the scale of the score for a normalisation length (host code, no GPU needed)."""
    return float(_lib.load().th_tm_d0(int(norm_length)))


def seed_count(n_valid: int) -> int:
    """The seeds of a pair with ``n_valid`` valid positions: every start of every window length n_valid, n_valid div 2, ... >= 4."""
    m, W, seeds = int(n_valid), int(n_valid), 0
    while W >= 1:
        seeds += m - W + 1
        if W // 2 < 4:
            break
        W //= 2
    return seeds


def tmscore_arrays(ref_xyz, mob_xyz, offsets, norm_len=None, rounds: int = ROUNDS, device: int = 0, timing: Optional[dict] = None,
                   transform: bool = False, dist: bool = True) -> TmTables:
    """One th_tmscore call.  ``ref_xyz`` / ``mob_xyz`` [total, 3] float64, ``offsets`` [pairs + 1], ``norm_len`` None or [pairs].
    ``timing``: a dict whose ``kernel_ms`` grows by the device time of the kernels."""
    ref_xyz = np.ascontiguousarray(ref_xyz, dtype=np.float64).reshape(-1, 3)
    mob_xyz = np.ascontiguousarray(mob_xyz, dtype=np.float64).reshape(-1, 3)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    if offsets.size < 1:
        raise ValueError("offsets needs at least one entry")
    if ref_xyz.shape != mob_xyz.shape:
        raise ValueError(f"ref_xyz has {ref_xyz.shape[0]} positions, mob_xyz {mob_xyz.shape[0]}")
    total, n_pairs = ref_xyz.shape[0], offsets.size - 1
    if norm_len is not None:
        wanted = np.asarray(norm_len).reshape(-1)
        if wanted.size != n_pairs:
            raise ValueError(f"norm_len has {wanted.size} entries for {n_pairs} pairs")
        if wanted.size and (wanted.min() < 0 or wanted.max() > np.iinfo(np.int32).max):
            raise ValueError("norm_len does not fit 0 .. 2^31 - 1")
        norm_len = np.ascontiguousarray(wanted, dtype=np.int32)
    tm = np.empty((n_pairs, 2), np.float64)
    counts = np.empty((n_pairs, 4), np.int64)
    d = np.empty(total, np.float64) if dist else None
    moves = np.empty((n_pairs, 3, 4), np.float64) if transform else None
    ms = C.c_double(0.0)
    _lib.check(_lib.load().th_tmscore(int(device), ptr(ref_xyz), ptr(mob_xyz), total, ptr(offsets), n_pairs, ptr(norm_len), int(rounds), ptr(tm),
                                      ptr(counts), ptr(d), ptr(moves), C.byref(ms) if timing is not None else None))
    if timing is not None:
        timing["kernel_ms"] = timing.get("kernel_ms", 0.0) + ms.value
    return TmTables(tm, counts, d, moves)


@dataclass
class TmResult:
    error: Optional[str]               # why the pair was not scored (every figure below is then NaN / 0 / empty)
    tm: float
    d0: float
    n_valid: int
    norm_length: int                   # L: the reference's residues that have the atom
    n_seeds: int
    n_fits: int
    dist: np.ndarray                   # [paired positions] float64: d_i under the best superposition
    residues: List[pdbio.Residue]      # the REFERENCE's residue of each paired position
    unpaired_reference: int
    unpaired_model: int
    transform: Optional[np.ndarray] = None     # [3, 4], when asked for


def _failed(error: str) -> TmResult:
    nan = float("nan")
    return TmResult(error, nan, nan, 0, 0, 0, 0, np.zeros(0, np.float64), [], 0, 0)


def _valid_count(ref, mod, ours, theirs) -> int:
    return int((np.isfinite(ref.xyz[ours]).all(axis=1) & np.isfinite(mod.xyz[theirs]).all(axis=1)).sum()) if len(ours) else 0


def tmscore(pairs: Sequence[Tuple], pair_by: str = "position", atom: str = "CA", rounds: int = ROUNDS, device: int = 0, transform: bool = False,
            workers: int = 8, budget_bytes: int = structure.BATCH_BYTES, stats: Optional[dict] = None) -> List[TmResult]:
    """Every ``(reference, model)`` pair — paths of PDB files (plain or gzipped), ``pdbio.Model`` objects or ``AtomLayout`` objects, as
    for ``superpose.superpose`` — scored under the rule of the module docstring.  One GPU call per batch; a pair is charged its
    positions AND its seeds against ``budget_bytes`` (60 bytes per position, 12 per seed: a pair of 300 has 1514 seeds).  A pair that
    cannot be scored — more than 4096 positions among them — carries its ``error`` and does not stop the others.  ``stats``
    receives ``submissions``, ``kernel_ms`` and ``files_parsed``.  ``pairs`` may be what ``superpose.prepare`` returned."""
    if int(rounds) < 0:
        raise ValueError(f"rounds = {rounds} is negative")
    prepared = prepare(pairs, pair_by, atom, workers)
    pairs_ok = [f"{len(item[2])} paired positions: th_tmscore takes {MAX_POSITIONS} at most" if not isinstance(item, str) and len(item[2]) > MAX_POSITIONS
                else item for item in prepared.pairs]
    todo = Prepared(pairs_ok, prepared.files, prepared.atom, prepared.counted)

    def arrays(ref_xyz, mob_xyz, offsets, timing, part):
        norm_len = np.array([len(ref.residues) for ref, _, _, _ in part], dtype=np.int32)
        return tmscore_arrays(ref_xyz, mob_xyz, offsets, norm_len, rounds, device, timing, transform, True)

    def result(got, j, a, b, ref, mod, ours, theirs):
        counts = got.counts[j]
        return TmResult(None, float(got.tm[j, 0]), float(got.tm[j, 1]), int(counts[0]), int(counts[1]), int(counts[2]), int(counts[3]),
                        got.dist[a:b].copy(), [ref.residues[i] for i in ours], len(ref.residues) - len(ours), len(mod.residues) - len(theirs),
                        got.transform[j].copy() if transform else None)
    # charged in bytes: a pair costs its positions and its seeds, which follow from its valid positions
    return score_pairs(todo, budget_bytes, stats, 1, arrays, result, _failed,
                       cost=lambda ref, mod, ours, theirs: pair_bytes(len(ours), _valid_count(ref, mod, ours, theirs)), whole_pairs=True)


def pair_bytes(n_positions: int, n_valid: int) -> int:
    """What a pair takes of the byte budget: its positions and its seeds."""
    return int(n_positions) * _POSITION_BYTES + seed_count(n_valid) * _SEED_BYTES
