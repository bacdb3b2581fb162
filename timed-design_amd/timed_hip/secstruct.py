"""Secondary structure of PDB structures, batched on the GPU: where the helices and strands are, by the DSSP rule (Kabsch & Sander
1983), through th_secondary_structure (csrc/secstruct.hip): an all-pairs float64 pass over the residues of each structure for the
backbone hydrogen bonds, then integer pattern matching, every structure of a batch in one call.  The first thing anyone checks on a
refolded design is whether it kept the native's secondary structure; the reference leaves that to PyMOL pictures.

    *** PARITY UNPINNED AGAINST DSSP ***  (``mkdssp``, PyMOL's ``dss``, STRIDE.)  None of them is available where this project is
    built.  The rule is this project's reading of the published definition and not their code; it is written out in
    include/timed_hip.h.  Those programs' tie rules, bulges, G / I precedence and bond caps differ in detail: assignments can differ
    at helix ends and sheet edges.

    Per structure, residues 0 .. L-1 in file order, each with N, CA, C, O (float64), a chain id and a ``no_h`` flag (proline):

    * valid(i): all 12 coordinates are finite.  An invalid residue makes no bond, is a break on both sides and gets class ``-``;
    * conn(i), the link i -> i+1: both valid, the same chain id, squared C(i)-N(i+1) distance <= 6.25;
    * H(i) = N(i) + v / |v| with v = C(i-1) - O(i-1): only where conn(i-1) holds and ``no_h`` is false;
    * energy of acceptor a (C=O) and donor d (N-H), for a valid, d with H, d != a, d != a+1 and squared CA-CA distance < 81:
      q = ((1/rON + 1/rCH) - 1/rOH) - 1/rCN, e = floor(27.888 q 1000 + 0.5) milli-kcal/mol, -9900 when a distance is < 0.5 and never
      below; hb(a, d) <=> e < -500.  All bonds count: no "two best per residue" cap;
    * turn_n(i), n = 3, 4, 5: hb(i, i+n) and conn(i) .. conn(i+n-1); two consecutive n-turns make a helix (H for 4 at i .. i+3, G for 3
      at i .. i+2, I for 5 at i .. i+4); turn_n(i) makes T at i+1 .. i+n-1;
    * bridges, for |i - j| >= 3 with conn(i-1), conn(i), conn(j-1), conn(j), chains may differ:
      parallel <=> [hb(i-1, j) and hb(j, i+1)] or [hb(j-1, i) and hb(i, j+1)];
      antiparallel <=> [hb(i, j) and hb(j, i)] or [hb(i-1, j+1) and hb(j-1, i+1)];
    * E: a bridge (i, j) continued by a bridge of the same kind at (i+1, j+1) / (i-1, j-1) (parallel) or (i+1, j-1) / (i-1, j+1)
      (antiparallel); a bridged residue that is not E is B.  Beta-bulges are not bridged over; sheets are not labelled;
    * S: conn(i-2) .. conn(i+1) hold and the CA(i-2) -> CA(i) -> CA(i+2) direction changes by more than 70 degrees;
    * priority H > E > B > G > I > T > S > ``-``; codes 0 ``-``, 1 H, 2 B, 3 E, 4 G, 5 I, 6 T, 7 S; three states: H, G, I -> helix (H), E,
      B -> strand (E), the rest -> coil (C).

Structures are read as ``timed_hip.structure`` reads them: the first model, the first alternate location, the non-hetero residues,
chains in file order (a chain that comes back later in the file continues its entry), a missing backbone atom NaN.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import List, NamedTuple, Optional, Sequence, Union

import numpy as np

from . import _lib, batching, pdbio, structure
from ._lib import ptr

LETTERS = "-HBEGITS"                   # the letter of each class code
THREE_STATE = "CHEEHHCC"               # the three-state letter of each class code
FLAG_TURN3, FLAG_TURN4, FLAG_TURN5, FLAG_BEND, FLAG_PARALLEL, FLAG_ANTIPARALLEL, FLAG_CONN, FLAG_VALID = (1 << b for b in range(8))
_BACKBONE = ("N", "CA", "C", "O")
_RESIDUE_BYTES = 12 * 8 + 4 + 1 + 1 + 6 * 4    # backbone, chain, no_h, class and the row of residue_out


class SecondaryTables(NamedTuple):
    """What one th_secondary_structure call returns."""
    cls: np.ndarray                    # [total] uint8
    residue: np.ndarray                # [total, 6] int32: partner, partner, flags, bonds accepted, bonds donated, bridge partners
    structure: np.ndarray              # [S, 10] int64: n_valid, n_hbonds, the eight class counts
    bits: Optional[np.ndarray]         # [sum L * ceil(L / 64)] uint64, or None when not asked for


def bitmap_words(lengths) -> np.ndarray:
    """L * ceil(L / 64) for every length: the 64-bit words of a structure's hydrogen-bond bitmap"""
    lengths = np.asarray(lengths, dtype=np.int64)
    return lengths * ((lengths + 63) // 64)


def structure_bytes(length: int) -> int:
    """what a structure of ``length`` residues takes in one call: its arrays and its bitmap"""
    return int(length) * _RESIDUE_BYTES + int(bitmap_words(length)) * 8


def secondary_structure_arrays(backbone, chain, no_h, offsets, device: int = 0, bits: bool = False,
                               timing: Optional[dict] = None) -> SecondaryTables:
    """One th_secondary_structure call.  ``backbone`` [total, 4, 3] float64 (N, CA, C, O), ``chain`` [total] int32, ``no_h`` [total]
    uint8, ``offsets`` [S + 1].  ``bits``: also return the hydrogen-bond bitmaps.  ``timing``: a dict whose ``kernel_ms`` grows by the
    device time of the kernels and whose ``hbonds_ms``, ``assign_ms`` and ``totals_ms`` grow by that of each."""
    backbone = np.ascontiguousarray(backbone, dtype=np.float64).reshape(-1, 4, 3)
    chain = np.ascontiguousarray(chain, dtype=np.int32).reshape(-1)
    no_h = np.ascontiguousarray(no_h, dtype=np.uint8).reshape(-1)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    if offsets.size < 1:
        raise ValueError("offsets needs at least one entry")
    total, n_structures = backbone.shape[0], offsets.size - 1
    if chain.size != total or no_h.size != total:
        raise ValueError(f"chain and no_h need {total} entries")
    cls = np.empty(total, np.uint8)
    residue = np.empty((total, 6), np.int32)
    per_structure = np.empty((n_structures, 10), np.int64)
    words = None
    if bits:
        if np.any(np.diff(offsets) < 0):
            raise ValueError("offsets decrease")
        words = np.empty(int(bitmap_words(np.diff(offsets)).sum()), np.uint64)
    ms = (C.c_double * 3)(0.0, 0.0, 0.0)
    _lib.check(_lib.load().th_secondary_structure(int(device), ptr(backbone), ptr(chain), ptr(no_h), total, ptr(offsets), n_structures, ptr(cls),
                                                  ptr(residue), ptr(per_structure), ptr(words),
                                                  C.cast(ms, C.POINTER(C.c_double)) if timing is not None else None))
    if timing is not None:
        timing["kernel_ms"] = timing.get("kernel_ms", 0.0) + sum(ms)
        for key, value in zip(("hbonds_ms", "assign_ms", "totals_ms"), ms):
            timing[key] = timing.get(key, 0.0) + value
    return SecondaryTables(cls, residue, per_structure, words)


@dataclass
class BackboneLayout:
    """One structure as th_secondary_structure takes it."""
    backbone: np.ndarray               # [n, 4, 3] float64: N, CA, C, O, NaN where the residue lacks the atom
    chain: np.ndarray                  # [n] int32: chains numbered in order of appearance
    no_h: np.ndarray                   # [n] uint8: 1 for PRO
    residues: List[pdbio.Residue]


def backbone_layout(model: pdbio.Model, all_chains: bool = True) -> BackboneLayout:
    """The non-hetero residues, chains in file order (``all_chains=False``: the first chain): their backbone atoms, chain ids numbered
    in order of appearance, ``no_h`` for PRO, NaN for a missing atom."""
    members: dict = {}
    for r in structure.reported_residues(model, all_chains):
        members.setdefault(r.chain, []).append(r)
    return layout_of_residues([r for chain in members.values() for r in chain])


def layout_of_residues(residues: Sequence[pdbio.Residue]) -> BackboneLayout:
    """The residues as they come: chain ids numbered in order of appearance, ``no_h`` for PRO, NaN for a missing atom."""
    residues = list(residues)
    backbone = np.full((len(residues), 4, 3), np.nan)
    chain_id = np.zeros(len(residues), np.int32)
    numbers: dict = {}
    for k, res in enumerate(residues):
        for a, name in enumerate(_BACKBONE):
            if name in res.atoms:
                backbone[k, a] = res.atoms[name]
        chain_id[k] = numbers.setdefault(res.chain, len(numbers))
    return BackboneLayout(backbone, chain_id, np.array([r.name == "PRO" for r in residues], dtype=np.uint8), residues)


@dataclass
class StructureSecondary:
    error: Optional[str]               # why the structure was not assigned (everything below is then empty / 0)
    cls: np.ndarray                    # [residues] uint8 class codes
    partners: np.ndarray               # [residues, 2] int32: the two lowest bridge partners (indices into ``residues``) or -1
    flags: np.ndarray                  # [residues] int32 (FLAG_*)
    accepted: np.ndarray               # [residues] int32: hydrogen bonds of the residue's C=O
    donated: np.ndarray                # [residues] int32: hydrogen bonds of the residue's N-H
    n_partners: np.ndarray             # [residues] int32
    n_valid: int
    n_hbonds: int
    counts: np.ndarray                 # [8] int64: residues of each class
    residues: List[pdbio.Residue]

    @property
    def string(self) -> str:
        return as_string(self.cls)

    @property
    def fractions(self):
        """(helix, strand, coil) shares of the residues; NaN for an empty structure"""
        return state_fractions(self.counts)


def state_fractions(counts):
    """the helix (H + G + I), strand (E + B) and coil shares of the eight class counts; NaN when there is no residue"""
    c = [int(v) for v in counts]
    n = sum(c)
    if n == 0:
        return float("nan"), float("nan"), float("nan")
    helix, strand = c[1] + c[4] + c[5], c[2] + c[3]
    return helix / n, strand / n, (n - helix - strand) / n


def _failed(error: str) -> StructureSecondary:
    none = np.zeros(0, np.int32)
    return StructureSecondary(error, np.zeros(0, np.uint8), np.zeros((0, 2), np.int32), none, none, none, none, 0, 0, np.zeros(8, np.int64), [])


def three_state(codes) -> np.ndarray:
    """class codes -> 0 coil, 1 helix (H, G, I), 2 strand (E, B), uint8"""
    table = np.array([0, 1, 2, 2, 1, 1, 0, 0], np.uint8)
    return table[np.asarray(codes, dtype=np.int64)]


def as_string(codes, three: bool = False) -> str:
    """class codes as letters (``-HBEGITS``); ``three``: the three-state letters H, E, C"""
    letters = THREE_STATE if three else LETTERS
    return "".join(letters[c] for c in np.asarray(codes, dtype=np.int64).reshape(-1).tolist())


def secondary_structure_layouts(layouts: Sequence[BackboneLayout], device: int = 0, budget_bytes: int = batching.BATCH_BYTES,
                                stats: Optional[dict] = None) -> List[StructureSecondary]:
    """The layouts through th_secondary_structure in as few calls as ``budget_bytes`` allows; a structure is charged its arrays AND its
    hydrogen-bond bitmap (``structure_bytes``).  ``stats`` receives ``submissions`` and ``kernel_ms``."""
    out: List[StructureSecondary] = []

    def submit(part, timing):
        offsets = np.zeros(len(part) + 1, np.int64)
        np.cumsum([len(l.residues) for l in part], out=offsets[1:])
        got = secondary_structure_arrays(np.concatenate([l.backbone for l in part]), np.concatenate([l.chain for l in part]),
                                         np.concatenate([l.no_h for l in part]), offsets, device, timing=timing)
        for k, l in enumerate(part):
            a, b = int(offsets[k]), int(offsets[k + 1])
            rows, totals = got.residue[a:b], got.structure[k]
            out.append(StructureSecondary(None, got.cls[a:b].copy(), rows[:, :2].copy(), rows[:, 2].copy(), rows[:, 3].copy(), rows[:, 4].copy(),
                                          rows[:, 5].copy(), int(totals[0]), int(totals[1]), totals[2:].copy(), l.residues))
    batching.run_batches(layouts, [structure_bytes(len(l.residues)) for l in layouts], budget_bytes, 1, submit, stats)
    return out


def secondary_structure(files_or_models: Sequence[Union[pdbio.Model, BackboneLayout, str, os.PathLike]], device: int = 0,
                        budget_bytes: int = batching.BATCH_BYTES, workers: int = 8, stats: Optional[dict] = None) -> List[StructureSecondary]:
    """The secondary structure of every structure (``pdbio.Model`` objects, ``BackboneLayout`` objects or paths of PDB files, plain or
    gzipped) under the rule of the module docstring.  Files are parsed on ``workers`` host threads; one GPU call per batch, batches cut
    under ``budget_bytes`` with the bitmap counted in a structure's size.  A file that cannot be read carries its ``error`` and does
    not stop the others.  ``stats`` receives ``submissions``, ``kernel_ms`` and ``files_parsed``."""
    def parse(item):
        if isinstance(item, BackboneLayout):
            return item
        try:
            return backbone_layout(structure.first_model(item))
        except (OSError, EOFError, ValueError) as e:
            return f"{type(e).__name__}: {e}"
    items = list(files_or_models)
    parsed = batching.parse_each(parse, items, workers)
    good = [p for p in parsed if not isinstance(p, str)]
    if stats is not None:
        stats["files_parsed"] = stats.get("files_parsed", 0) + sum(1 for item in items if not isinstance(item, (BackboneLayout, pdbio.Model)))
    assigned = iter(secondary_structure_layouts(good, device, budget_bytes, stats))
    return [_failed(p) if isinstance(p, str) else next(assigned) for p in parsed]
