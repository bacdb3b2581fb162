"""Sequence alignment of models to their native, batched on the GPU, through th_seqalign (csrc/seqalign.hip): the pairing of a model
with its native that survives renumbering, a missing loop and a purification tag together — and that exists for a misfolded model too,
where the structural alignment of ``timed_hip.cealign`` finds nothing.  The reference's scripts/analyse_af2.py gets it one pair at a
time from PyMOL's ``cmd.align``, a sequence alignment followed by a fit; ``timed_hip.superpose`` is that fit, and ``prepare_aligned``
hands this alignment to it, to ``lddt.lddt``, ``tmscore.tmscore`` and every other scorer that takes a ``superpose.Prepared``.

    *** PARITY UNPINNED AGAINST PYMOL ***  PyMOL is not available where this project is built, and ``cmd.align``'s own recurrences,
    end-gap treatment and tie handling are not available to pin against.  The rule is this project's own, written out in
    include/timed_hip.h: a global alignment with affine gap costs (three tables H, E, F), in integers; a run of k unpaired residues
    costs ``gap_open + (k - 1) gap_extend``; the ends are free (``free_ends=True``, the default) or charged; on equal scores the
    diagonal is kept before a gap in the reference before a gap in the model, a gap is opened before it is extended, and the end
    cell nearest the corner wins.

    * a residue is one byte: 0..19 the letters of ``analysis.RESIDUES``, 20 anything else (the coding of ``seqset.encode``); residue
      names map to letters through ``design_utils.amino_acids.standard_amino_acids``;
    * the substitution table is an input of the call: ``default_matrix()`` is 2 x BLOSUM62 with -2 wherever either code is 20, which
      makes ``cmd.align``'s documented ``gap=-10, extend=-0.5`` the integers 20 and 1.  ``score`` is in units of the table: halve it
      for BLOSUM62 units;
    * structures are read exactly as ``timed_hip.superpose`` reads them; chains are concatenated in ``atom_layout`` order and one
      alignment is made per pair;
    * a sequence of more than ``MAX_LENGTH`` (4096) residues is its pair's ``error``.

Out of scope: local (Smith-Waterman) alignment, profile or multiple alignment, banded or heuristic search, TM-align.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _lib, analysis, batching, pdbio, seqset, structure
from ._lib import ptr
from .superpose import AtomLayout, Prepared, _load_layouts

MAX_LENGTH = 4096                  # TH_SEQALIGN_MAX_LENGTH
GAP_OPEN, GAP_EXTEND = 20, 1       # cmd.align's -10 and -0.5 in units of default_matrix()
UNKNOWN = seqset.UNKNOWN
COUNT_COLUMNS = ("n_ref", "n_model", "score", "n_aligned", "n_identical", "n_positive", "n_gaps", "n_gap_residues")
_STRIP, _LANES = 8, 64             # columns per lane and lanes per panel of k_seqalign_fill
_REF_BYTES, _MODEL_BYTES, _PAIR_BYTES = 17, 5, 120


def default_matrix() -> np.ndarray:
    """int32 [21, 21]: 2 x ``analysis.BLOSUM62``, and -2 wherever either code is 20"""
    table = np.full((21, 21), -2, np.int32)
    table[:20, :20] = 2 * analysis.BLOSUM62.astype(np.int32)
    return table


_CODE_OF_NAME = None


def codes_of_names(names: Sequence[str]) -> np.ndarray:
    """uint8 codes of three-letter residue names through ``standard_amino_acids``; an unknown name is 20"""
    global _CODE_OF_NAME
    if _CODE_OF_NAME is None:
        from design_utils.amino_acids import standard_amino_acids
        _CODE_OF_NAME = {three: analysis.RESIDUES.index(letter) for letter, three in standard_amino_acids.items()}
    return np.array([_CODE_OF_NAME.get(str(name).strip().upper(), UNKNOWN) for name in names], np.uint8)


def codes_of_string(sequence: str) -> np.ndarray:
    """uint8 codes of a string of one-letter codes: the coding of ``seqset.encode``"""
    return seqset.encode([sequence])[0]


class SeqalignTables(NamedTuple):
    """What one th_seqalign call returns."""
    align: np.ndarray                  # [ref_total] int32: the model residue, local to the pair, aligned to this reference residue; -1 if none
    counts: np.ndarray                 # [pairs, 8] int64: COUNT_COLUMNS


def seqalign_arrays(ref_codes, ref_offsets, mob_codes, mob_offsets, matrix=None, gap_open: int = GAP_OPEN, gap_extend: int = GAP_EXTEND,
                    free_ends: bool = True, device: int = 0, timing: Optional[dict] = None) -> SeqalignTables:
    """One th_seqalign call.  ``ref_codes`` and ``mob_codes`` flat uint8, each with its own ``offsets`` [pairs + 1]; ``matrix`` int32
    [21, 21] (``default_matrix()`` when None).  ``timing``: a dict whose ``kernel_ms`` grows by the device time of both kernels,
    ``fill_ms`` and ``trace_ms`` by that of each."""
    ref_codes = np.ascontiguousarray(ref_codes, dtype=np.uint8).reshape(-1)
    mob_codes = np.ascontiguousarray(mob_codes, dtype=np.uint8).reshape(-1)
    ref_offsets = np.ascontiguousarray(ref_offsets, dtype=np.int64).reshape(-1)
    mob_offsets = np.ascontiguousarray(mob_offsets, dtype=np.int64).reshape(-1)
    if ref_offsets.size < 1 or ref_offsets.size != mob_offsets.size:
        raise ValueError(f"ref_offsets has {ref_offsets.size} entries, mob_offsets {mob_offsets.size}: both need pairs + 1")
    matrix = np.ascontiguousarray(default_matrix() if matrix is None else matrix, dtype=np.int32)
    if matrix.shape != (21, 21):
        raise ValueError(f"matrix has shape {matrix.shape}, not (21, 21)")
    n_pairs = ref_offsets.size - 1
    align = np.empty(ref_codes.size, np.int32)
    counts = np.empty((n_pairs, 8), np.int64)
    ms = (C.c_double * 2)(0.0, 0.0)
    _lib.check(_lib.load().th_seqalign(int(device), ptr(ref_codes), ref_codes.size, ptr(ref_offsets), ptr(mob_codes), mob_codes.size,
                                       ptr(mob_offsets), n_pairs, ptr(matrix), int(gap_open), int(gap_extend), int(bool(free_ends)), ptr(align),
                                       ptr(counts), C.cast(ms, C.POINTER(C.c_double)) if timing is not None else None))
    if timing is not None:
        timing["kernel_ms"] = timing.get("kernel_ms", 0.0) + ms[0] + ms[1]
        timing["fill_ms"] = timing.get("fill_ms", 0.0) + ms[0]
        timing["trace_ms"] = timing.get("trace_ms", 0.0) + ms[1]
    return SeqalignTables(align, counts)


@dataclass
class SeqalignResult:
    error: Optional[str]               # why the pair was not aligned (every figure below is then 0 / empty)
    n_ref: int
    n_model: int
    score: int                         # in units of the table
    n_aligned: int
    n_identical: int
    n_positive: int
    n_gaps: int
    n_gap_residues: int
    reference_index: np.ndarray        # [n_aligned] int64: positions of the reference, ascending
    model_index: np.ndarray            # [n_aligned] int64: the model position aligned to each
    reference: Optional[AtomLayout] = None
    model: Optional[AtomLayout] = None

    def _over(self, count: int, by: int) -> float:
        return count / by if by > 0 else float("nan")

    @property
    def identity(self) -> float:
        return self._over(self.n_identical, self.n_aligned)

    @property
    def positives(self) -> float:
        return self._over(self.n_positive, self.n_aligned)

    @property
    def coverage_ref(self) -> float:
        return self._over(self.n_aligned, self.n_ref)

    @property
    def coverage_model(self) -> float:
        return self._over(self.n_aligned, self.n_model)


def _failed(error: str) -> SeqalignResult:
    return SeqalignResult(error, 0, 0, 0, 0, 0, 0, 0, 0, np.zeros(0, np.int64), np.zeros(0, np.int64))


def trace_bytes(n_ref: int, n_model: int) -> int:
    """the trace bits of one pair on the device: a dword per (step, strip of 8 columns) of every panel of 64 strips"""
    n, m = int(n_ref), int(n_model)
    if n == 0 or m == 0:
        return 0
    panel = _STRIP * _LANES
    panels = (m + panel - 1) // panel
    strips = (m - (panels - 1) * panel + _STRIP - 1) // _STRIP
    return 4 * ((panels - 1) * (n + _LANES - 1) * _LANES + (n + strips - 1) * strips)


def pair_bytes(n_ref: int, n_model: int) -> int:
    """What a pair takes of the byte budget: its trace storage plus its positions"""
    return trace_bytes(n_ref, n_model) + _REF_BYTES * int(n_ref) + _MODEL_BYTES * int(n_model) + _PAIR_BYTES


def _check_costs(gap_open, gap_extend):
    if int(gap_open) != gap_open or int(gap_extend) != gap_extend or not 0 <= int(gap_extend) <= int(gap_open) <= 32767:
        raise ValueError(f"gap_open = {gap_open} and gap_extend = {gap_extend} must be integers with 0 <= gap_extend <= gap_open <= 32767")


def _align_codes(jobs, results, make, matrix, gap_open, gap_extend, free_ends, device, budget_bytes, stats):
    """``jobs``: (k, reference codes, model codes, ...) — one call per batch; ``results[k] = make(job, counts row, ours, theirs)``"""
    def submit(part, timing):
        ref_offsets = np.zeros(len(part) + 1, np.int64)
        mob_offsets = np.zeros(len(part) + 1, np.int64)
        np.cumsum([len(job[1]) for job in part], out=ref_offsets[1:])
        np.cumsum([len(job[2]) for job in part], out=mob_offsets[1:])
        empty = [np.zeros(0, np.uint8)]
        got = seqalign_arrays(np.concatenate([job[1] for job in part] + empty), ref_offsets, np.concatenate([job[2] for job in part] + empty),
                              mob_offsets, matrix, gap_open, gap_extend, free_ends, device, timing)
        for j, job in enumerate(part):
            partner = got.align[int(ref_offsets[j]):int(ref_offsets[j + 1])]
            ours = np.nonzero(partner >= 0)[0].astype(np.int64)
            results[job[0]] = make(job, [int(c) for c in got.counts[j]], ours, partner[ours].astype(np.int64))
    batching.run_batches(jobs, [pair_bytes(len(job[1]), len(job[2])) for job in jobs], budget_bytes, 1, submit, stats)


def align(pairs: Sequence[Tuple], atom: str = "CA", matrix=None, gap_open: int = GAP_OPEN, gap_extend: int = GAP_EXTEND, free_ends: bool = True,
          device: int = 0, workers: int = 8, budget_bytes: int = structure.BATCH_BYTES, stats: Optional[dict] = None) -> List[SeqalignResult]:
    """Every ``(reference, model)`` pair — paths of PDB files (plain or gzipped), ``pdbio.Model`` objects or ``AtomLayout`` objects, as
    for ``superpose.superpose`` — aligned by sequence under the rule of the module docstring: the residues of either layout, in its
    order, are the two sequences.  Every distinct file is read once; one GPU call per batch; a pair is charged ``pair_bytes`` against
    ``budget_bytes``.  A pair that cannot be aligned — a structure of more than 4096 positions among them — carries its ``error`` and
    does not stop the others.  ``stats`` receives ``submissions``, ``kernel_ms`` and ``files_parsed``."""
    _check_costs(gap_open, gap_extend)
    sides = [side for pair in pairs for side in pair[:2]]
    flat = _load_layouts(sides, atom, workers)
    results: List[Optional[SeqalignResult]] = []
    coded, jobs = {}, []

    def codes(layout):
        if id(layout) not in coded:
            coded[id(layout)] = codes_of_names([r.name for r in layout.residues])
        return coded[id(layout)]
    for k, (ref, mod) in enumerate(zip(flat[0::2], flat[1::2])):
        broken = [side for side in (ref, mod) if isinstance(side, str)]
        longest = 0 if broken else max(len(ref.residues), len(mod.residues))
        if broken:
            results.append(_failed("; ".join(broken)))
        elif longest > MAX_LENGTH:
            results.append(_failed(f"{longest} positions in one structure: th_seqalign takes {MAX_LENGTH} at most"))
        else:
            results.append(None)
            jobs.append((k, codes(ref), codes(mod), ref, mod))
    _align_codes(jobs, results, lambda job, counts, ours, theirs: SeqalignResult(None, *counts, ours, theirs, job[3], job[4]), matrix, gap_open,
                 gap_extend, free_ends, device, budget_bytes, stats)
    if stats is not None:
        stats["files_parsed"] = stats.get("files_parsed", 0) + len({os.fspath(s) for s in sides if not isinstance(s, (AtomLayout, pdbio.Model))})
    return results


def align_strings(pairs: Sequence[Tuple[str, str]], matrix=None, gap_open: int = GAP_OPEN, gap_extend: int = GAP_EXTEND, free_ends: bool = True,
                  device: int = 0, budget_bytes: int = structure.BATCH_BYTES, stats: Optional[dict] = None) -> List[SeqalignResult]:
    """The same for plain sequences: ``(reference, model)`` strings of one-letter codes (any other character is code 20)"""
    _check_costs(gap_open, gap_extend)
    results: List[Optional[SeqalignResult]] = []
    jobs = []
    for k, (ref, mod) in enumerate(pairs):
        longest = max(len(ref), len(mod))
        if longest > MAX_LENGTH:
            results.append(_failed(f"{longest} residues in one sequence: th_seqalign takes {MAX_LENGTH} at most"))
        else:
            results.append(None)
            jobs.append((k, codes_of_string(ref), codes_of_string(mod)))
    _align_codes(jobs, results, lambda job, counts, ours, theirs: SeqalignResult(None, *counts, ours, theirs), matrix, gap_open, gap_extend,
                 free_ends, device, budget_bytes, stats)
    return results


def gapped(reference: str, model: str, result: SeqalignResult) -> Tuple[str, str]:
    """the two sequences written over one another with '-' where a residue has no partner, end to end"""
    top, bottom, i, j = [], [], 0, 0
    for p, q in zip(result.reference_index.tolist() + [len(reference)], result.model_index.tolist() + [len(model)]):
        top.append(reference[i:p] + "-" * (q - j))
        bottom.append("-" * (p - i) + model[j:q])
        if p < len(reference):
            top.append(reference[p])
            bottom.append(model[q])
        i, j = p + 1, q + 1
    return "".join(top), "".join(bottom)


def prepare_aligned(pairs: Sequence[Tuple], results: Optional[List[SeqalignResult]] = None, atom: str = "CA", matrix=None,
                    gap_open: int = GAP_OPEN, gap_extend: int = GAP_EXTEND, free_ends: bool = True, device: int = 0, workers: int = 8,
                    budget_bytes: int = structure.BATCH_BYTES, stats: Optional[dict] = None) -> Prepared:
    """A ``superpose.Prepared`` whose index pairs are the sequence alignment of every pair: ``superpose.superpose``, ``lddt.lddt``,
    ``tmscore.tmscore`` and the others then score the aligned positions unchanged (what either side has alone counts as unpaired).
    A pair with an ``error`` keeps it.  ``results``: what ``align`` already returned for the same pairs — nothing is aligned twice."""
    if results is None:
        results = align(pairs, atom, matrix, gap_open, gap_extend, free_ends, device, workers, budget_bytes, stats)
    sides = [side for pair in pairs for side in pair[:2]]
    out = [res.error if res.error else (res.reference, res.model, res.reference_index, res.model_index) for res in results]
    prepared = Prepared(out, len({os.fspath(s) for s in sides if not isinstance(s, (AtomLayout, pdbio.Model))}), atom)
    if stats is not None:
        prepared.counted.append(stats)                                 # align() counted the files already
    return prepared
