"""lDDT of models against their native, batched on the GPU: the local Distance Difference Test (Mariani et al. 2013) of every
(reference, model) pair, per position and per pair, through th_lddt (csrc/lddt.hip): an all-pairs float64 kernel, every pair of a
batch in one launch.  lDDT is the MEASURED counterpart of the pLDDT that AlphaFold2 predicts and writes into the B-factor column of
its models (the reference plots that prediction in ``plot_af2IDDT_vs_position``); it needs no fit of one structure on the other.

    *** PARITY UNPINNED AGAINST OPENSTRUCTURE ***  Neither OpenStructure nor AlphaFold's ``lddt.py`` is available where this project is
    built.  The rule is this project's reading of the published definition in the CA-only form AlphaFold uses, written out in
    include/timed_hip.h: one position per residue, no stereochemistry checks, strict inequalities on both tests.  For every position
    i, the positions j != i closer than ``radius`` (15 Angstrom) IN THE REFERENCE are its included pairs; a pair is preserved at a
    threshold t (0.5, 1, 2, 4 Angstrom) when the model's distance differs from the reference's by less than t.  ``lddt_i`` is the mean
    over the four thresholds of the preserved fraction of i's pairs; ``lddt`` is the same over ALL ordered pairs of the structure —
    pair-weighted, not the mean of ``lddt_i``.  No sequence alignment is made.

    * structures are read and positions are paired exactly as ``timed_hip.superpose`` does (``pair_by="position"`` or ``"number"``);
    * a position with a non-finite coordinate in either structure is neither an i nor a j;
    * MIRROR IMAGES: a mirror image has the distances of the original, so it scores 1.0 here, where the fit of ``superpose`` reports
      10.7 Angstrom for the mirrored 1ubq; a re-oriented domain, on the other hand, ruins that one global fit and costs lDDT only the
      pairs across the hinge.  That is the reason to report both;
    * ``model_bfactor`` is the model's B-factor of the paired atom, as stored: for an AlphaFold2 model the pLDDT on its 0-100 scale.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _lib, pdbio, structure
from ._lib import ptr
from .superpose import _load_layouts, pair_positions, prepare, score_pairs  # noqa: F401  (the first two: read and paired exactly as there)

RADIUS = 15.0
THRESHOLDS = (0.5, 1.0, 2.0, 4.0)
_POSITION_BYTES = 2 * 3 * 8 + 5 * 4        # both coordinate lists and the row of counts: the O(L^2) distances never leave registers


class LddtTables(NamedTuple):
    """What one th_lddt call returns."""
    residue: np.ndarray                # [total, 5] int32: n_i, c_i[0..3]; zeros at an invalid position
    pair: np.ndarray                   # [pairs, 6] int64: n_valid, N, C[0..3] (ordered pairs)


def lddt_arrays(ref_xyz, mob_xyz, offsets, radius: float = RADIUS, thresholds: Sequence[float] = THRESHOLDS, device: int = 0,
                timing: Optional[dict] = None) -> LddtTables:
    """One th_lddt call.  ``ref_xyz`` / ``mob_xyz`` [total, 3] float64, ``offsets`` [pairs + 1].  ``timing``: a dict whose
    ``kernel_ms`` grows by the device time of the kernels."""
    ref_xyz = np.ascontiguousarray(ref_xyz, dtype=np.float64).reshape(-1, 3)
    mob_xyz = np.ascontiguousarray(mob_xyz, dtype=np.float64).reshape(-1, 3)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    limits = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
    if offsets.size < 1:
        raise ValueError("offsets needs at least one entry")
    if ref_xyz.shape != mob_xyz.shape:
        raise ValueError(f"ref_xyz has {ref_xyz.shape[0]} positions, mob_xyz {mob_xyz.shape[0]}")
    if limits.size != 4:
        raise ValueError(f"four thresholds are needed, got {limits.size}")
    total, n_pairs = ref_xyz.shape[0], offsets.size - 1
    residue = np.empty((total, 5), np.int32)
    pair = np.empty((n_pairs, 6), np.int64)
    ms = C.c_double(0.0)
    _lib.check(_lib.load().th_lddt(int(device), ptr(ref_xyz), ptr(mob_xyz), total, ptr(offsets), n_pairs, float(radius), ptr(limits),
                                   ptr(residue), ptr(pair), C.byref(ms) if timing is not None else None))
    if timing is not None:
        timing["kernel_ms"] = timing.get("kernel_ms", 0.0) + ms.value
    return LddtTables(residue, pair)


def fractions(counts) -> Tuple[Tuple[float, float, float, float], float]:
    """The four preserved fractions and their mean, the lDDT, from (n, c[0..3]): NaN when n = 0.  The mean is formed as
    sum_k c[k] / (4 n)."""
    n = int(counts[0])
    if n == 0:
        nan = float("nan")
        return (nan, nan, nan, nan), nan
    c = [int(v) for v in counts[1:5]]
    return tuple(v / n for v in c), sum(c) / (4 * n)


@dataclass
class LddtResult:
    error: Optional[str]               # why the pair was not scored (every figure below is then NaN / 0 / empty)
    n_valid: int
    n_included: int                    # N: ordered included pairs
    preserved: Tuple[float, float, float, float]       # C[k] / N at the four thresholds
    lddt: float                        # sum_k C[k] / (4 N): pair-weighted
    lddt_i: np.ndarray                 # [paired positions] float64, NaN where n_i = 0
    n_i: np.ndarray                    # [paired positions] int32
    residues: List[pdbio.Residue]      # the REFERENCE's residue of each paired position
    unpaired_reference: int
    unpaired_model: int
    model_bfactor: np.ndarray          # [paired positions] float64: the model's B-factor of the paired atom, NaN when absent


def _failed(error: str) -> LddtResult:
    nan = float("nan")
    return LddtResult(error, 0, 0, (nan, nan, nan, nan), nan, np.zeros(0, np.float64), np.zeros(0, np.int32), [], 0, 0, np.zeros(0, np.float64))


def lddt(pairs: Sequence[Tuple], pair_by: str = "position", atom: str = "CA", radius: float = RADIUS, thresholds: Sequence[float] = THRESHOLDS,
         device: int = 0, workers: int = 8, budget_bytes: int = structure.BATCH_BYTES, stats: Optional[dict] = None) -> List[LddtResult]:
    """Every ``(reference, model)`` pair — paths of PDB files (plain or gzipped), ``pdbio.Model`` objects or ``AtomLayout`` objects, as
    for ``superpose.superpose`` — scored under the rule of the module docstring.  One GPU call per batch; batches are cut by
    ``batching.cut_batches`` under ``budget_bytes`` (68 bytes per position: its coordinates and counts, nothing per pair of
    positions).  A pair that cannot be scored carries its ``error`` and does not stop the others.  ``stats`` receives
    ``submissions``, ``kernel_ms`` and ``files_parsed``.  ``pairs`` may be what ``superpose.prepare`` returned."""
    prepared = prepare(pairs, pair_by, atom, workers)

    def result(got, j, a, b, ref, mod, ours, theirs):
        rows, totals = got.residue[a:b], got.pair[j]
        preserved, whole = fractions(totals[1:6])
        n_i = rows[:, 0].copy()
        with np.errstate(invalid="ignore", divide="ignore"):
            lddt_i = np.where(n_i > 0, rows[:, 1:5].sum(axis=1) / (4.0 * n_i), np.nan)
        bfactor = np.array([mod.residues[t].bfactors.get(prepared.atom, float("nan")) for t in theirs], dtype=np.float64)
        return LddtResult(None, int(totals[0]), int(totals[1]), preserved, whole, lddt_i, n_i, [ref.residues[i] for i in ours],
                          len(ref.residues) - len(ours), len(mod.residues) - len(theirs), bfactor)
    return score_pairs(prepared, budget_bytes, stats, _POSITION_BYTES,
                       lambda ref_xyz, mob_xyz, offsets, timing: lddt_arrays(ref_xyz, mob_xyz, offsets, radius, thresholds, device, timing),
                       result, _failed)
