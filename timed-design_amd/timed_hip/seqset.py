"""Diversity and native recovery of sampled sequences, batched on the GPU, through th_seqset (csrc/seqset.hip): how close the draws of
``sample.py`` are to the native, how different they are from one another and which are the same sequence twice, which few to fold, and
what the ensemble looks like per position — every set of a batch in one call.  The reference reports the identity and the BLOSUM62
similarity of ONE sequence against the native (ui.py) and draws a sequence logo; the rest it leaves to the reader.

    A *set* is the N sequences drawn for one structure, all of one length L >= 1 (N = 0 is allowed).  A residue is one byte: codes
    0..19 are the letters of ``analysis.RESIDUES`` (ACDEFGHIKLMNPQRSTVWY), code 20 is any other letter.  M(i, j) is the number of
    positions at which sequences i and j hold the same byte (code 20 equals code 20).  The tables, all integers (the rule is written
    out in include/timed_hip.h):

    * per sequence, int32 [n, 8]: native_identical; native_similar (both codes below 20 and BLOSUM62[native][seq] > 0: the
      reference's similarity); native_score (the sum of BLOSUM62 over those positions); pair_sum = sum_{j != i} M(i, j);
      nearest_matches = max_{j != i} M(i, j) and nearest_index, the lowest j attaining it (-1 and -1 when N = 1); first_equal, the
      lowest j with M(i, j) = L (the self pair counts: i is a distinct sequence iff first_equal == i); cluster;
    * per position, int32 [L, 21]: how many sequences hold each code there — the sequence logo of the draws;
    * per set, int64 [4]: sum_{i<j} M(i, j), distinct sequences, clusters (-1 without), sum_i native_identical;
    * on request the N x N matrix of M.

    Clustering is greedy, in input order: sequence n joins the lowest-indexed representative r < n with M(n, r) >= min_matches,
    otherwise it becomes a representative.  It is the incremental scheme of CD-HIT-like tools in its plainest form — THIS PROJECT'S
    OWN RULE, NOT THEIR CODE: no word filter, no length sorting, no alignment.  ``cluster_identity`` is taken in per-mille,
    p = round(1000 * identity), and the device gets min_matches = ceil(p * L / 1000) in integer arithmetic (``min_matches_of``).

Identity is over all L positions; similarity, as the reference's formula is defined only where both letters are known, over those
positions (counted on the host).  Fractions, consensus (the lowest code on ties), entropy in bits and native recovery per position are
host arithmetic on these integers.

Out of scope: alignment of any kind, substitution scores between draws, sequence weighting, ranking by the physico-chemical metrics,
clustering orders other than the input order, plots.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from dataclasses import dataclass, field
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _lib, analysis, batching
from ._lib import ptr

LETTERS = analysis.RESIDUES + "X"      # the letter of codes 0 .. 20
UNKNOWN = 20
N_CODES = 21
SEQ_COLUMNS = ("native_identical", "native_similar", "native_score", "pair_sum", "nearest_matches", "nearest_index", "first_equal", "cluster")
SET_COLUMNS = ("pair_matches", "n_distinct", "n_clusters", "native_identical")
_CODE_OF = np.full(256, UNKNOWN, np.uint8)
for _k, _c in enumerate(analysis.RESIDUES):
    _CODE_OF[ord(_c)] = _k


class SeqsetTables(NamedTuple):
    """What one th_seqset call returns."""
    seq: np.ndarray                    # [sequences, 8] int32: SEQ_COLUMNS
    profile: np.ndarray                # [sum of L, 21] int32
    sets: np.ndarray                   # [S, 4] int64: SET_COLUMNS
    matrix: Optional[np.ndarray]       # [sum of N^2] int32, set after set, or None when not asked for


def tiles() -> Tuple[int, int, int]:
    """(sequences per row tile, sequences per column tile, positions per staged chunk) of the pair kernel (host code, no GPU needed)"""
    out = np.zeros(3, np.int32)
    _lib.check(_lib.load().th_seqset_tiles(ptr(out)))
    return tuple(int(v) for v in out)


def encode(sequences: Sequence[str]) -> np.ndarray:
    """[n, L] uint8 of equally long sequences: upper-cased, the letters of ``analysis.RESIDUES`` are 0..19, any other character is 20"""
    rows = [str(s).upper().encode("latin-1", "replace") for s in sequences]
    if len(set(len(r) for r in rows)) > 1:
        raise ValueError(f"sequences of unequal lengths ({sorted(set(len(r) for r in rows))})")
    length = len(rows[0]) if rows else 0
    return _CODE_OF[np.frombuffer(b"".join(rows), np.uint8)].reshape(len(rows), length)


def decode(codes) -> str:
    return "".join(LETTERS[c] for c in np.asarray(codes).tolist())


def min_matches_of(cluster_identity: float, length: int) -> int:
    """ceil(p * L / 1000) with p = round(1000 * identity), in integer arithmetic: 0.8 of 76 is 61"""
    p = int(round(1000.0 * float(cluster_identity)))
    if not 0 <= p <= 1000:
        raise ValueError(f"cluster_identity = {cluster_identity} is outside 0 .. 1")
    return (p * int(length) + 999) // 1000


def set_bytes(n: int, length: int, matrix: bool = False) -> int:
    """what one set takes in one call: its codes, 32 bytes per sequence out, native and profile row per position, and the matrix"""
    return n * length + 32 * n + 88 * length + (4 * n * n if matrix else 0)


def seqset_arrays(codes, seq_offsets, lengths, native=None, min_matches=None, substitution=None, matrix: bool = False, device: int = 0,
                  timing: Optional[dict] = None) -> SeqsetTables:
    """One th_seqset call.  ``codes`` flat uint8, ``seq_offsets`` [S + 1], ``lengths`` [S]; ``native`` flat uint8 [sum of L] or None;
    ``min_matches`` [S] int32 or None (no clustering); ``substitution`` defaults to ``analysis.BLOSUM62``.  ``timing``: a dict whose
    ``kernel_ms`` grows by the device time from the first kernel to the last, ``pairs_ms`` by that of the kernels before the clustering
    (pack, pairs, native, columns) and ``cluster_ms`` by that of k_seqset_cluster."""
    codes = np.ascontiguousarray(codes, dtype=np.uint8).reshape(-1)
    seq_offsets = np.ascontiguousarray(seq_offsets, dtype=np.int64).reshape(-1)
    lengths = np.ascontiguousarray(lengths, dtype=np.int32).reshape(-1)
    if seq_offsets.size != lengths.size + 1:
        raise ValueError(f"seq_offsets needs {lengths.size + 1} entries")
    n_sets, n_seq, n_pos = lengths.size, int(max(seq_offsets[-1], 0)), int(np.maximum(lengths, 0).astype(np.int64).sum())
    counts = np.diff(seq_offsets)
    if native is not None:
        native = np.ascontiguousarray(native, dtype=np.uint8).reshape(-1)
        if native.size != n_pos:
            raise ValueError(f"native needs {n_pos} entries")
        substitution = np.ascontiguousarray(analysis.BLOSUM62 if substitution is None else substitution, dtype=np.int8).reshape(-1)
        if substitution.size != 400:
            raise ValueError("substitution needs 20 x 20 entries")
    else:
        substitution = None
    if min_matches is not None:
        min_matches = np.ascontiguousarray(min_matches, dtype=np.int32).reshape(-1)
        if min_matches.size != n_sets:
            raise ValueError(f"min_matches needs {n_sets} entries")
    seq = np.empty((n_seq, 8), np.int32)
    profile = np.empty((n_pos, N_CODES), np.int32)
    sets = np.empty((n_sets, 4), np.int64)
    square = np.empty(int((counts * counts).sum()) if (counts >= 0).all() else 0, np.int32) if matrix else None
    ms = (C.c_double * 3)(0.0, 0.0, 0.0)
    _lib.check(_lib.load().th_seqset(int(device), ptr(codes), codes.size, ptr(seq_offsets), ptr(lengths), n_sets, ptr(native), ptr(substitution),
                                     ptr(min_matches), ptr(seq), ptr(profile), ptr(square), ptr(sets),
                                     C.cast(ms, C.POINTER(C.c_double)) if timing is not None else None))
    if timing is not None:
        timing["kernel_ms"] = timing.get("kernel_ms", 0.0) + sum(ms)
        timing["pairs_ms"] = timing.get("pairs_ms", 0.0) + ms[0]
        timing["cluster_ms"] = timing.get("cluster_ms", 0.0) + ms[1]
    return SeqsetTables(seq, profile, sets, square)


@dataclass
class SetResult:
    """One set, from the integers of th_seqset.  Fractions are float64 divisions of those integers; NaN where nothing is defined."""
    error: Optional[str]               # why the set was not scored (everything below is then empty / 0)
    n: int = 0
    length: int = 0
    seq: np.ndarray = field(default_factory=lambda: np.zeros((0, 8), np.int32))            # SEQ_COLUMNS
    profile: np.ndarray = field(default_factory=lambda: np.zeros((0, N_CODES), np.int32))
    totals: np.ndarray = field(default_factory=lambda: np.zeros(4, np.int64))              # SET_COLUMNS
    matrix: Optional[np.ndarray] = None                                                    # [n, n] int32 when asked for
    native: Optional[np.ndarray] = None                                                    # [length] uint8
    min_matches: int = -1
    known: Optional[np.ndarray] = None                                                     # [n] int32: positions with both letters known

    def _over(self, column: int, by: float) -> np.ndarray:
        return self.seq[:, column].astype(np.float64) / by if by > 0 else np.full(self.n, np.nan)

    @property
    def identity_to_native(self) -> np.ndarray:
        return self._over(0, float(self.length)) if self.native is not None else np.full(self.n, np.nan)

    @property
    def similarity_to_native(self) -> np.ndarray:
        """the reference's mean of (BLOSUM62 > 0) over the positions where it is defined: both letters known (host count ``known``)"""
        if self.native is None:
            return np.full(self.n, np.nan)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(self.known > 0, self.seq[:, 1].astype(np.float64) / self.known.astype(np.float64), np.nan)

    @property
    def native_score(self) -> np.ndarray:
        return self.seq[:, 2].astype(np.float64) if self.native is not None else np.full(self.n, np.nan)

    @property
    def mean_identity_to_others(self) -> np.ndarray:
        return self._over(3, float((self.n - 1) * self.length))

    @property
    def nearest_identity(self) -> np.ndarray:
        return self._over(4, float(self.length)) if self.n > 1 else np.full(self.n, np.nan)

    @property
    def nearest_index(self) -> np.ndarray:
        return self.seq[:, 5]

    @property
    def first_equal(self) -> np.ndarray:
        return self.seq[:, 6]

    @property
    def cluster(self) -> np.ndarray:
        return self.seq[:, 7]

    @property
    def mean_pairwise_identity(self) -> float:
        pairs = self.n * (self.n - 1) // 2
        return float(self.totals[0]) / float(pairs * self.length) if pairs > 0 else float("nan")

    @property
    def mean_identity_to_native(self) -> float:
        return float(self.totals[3]) / float(self.n * self.length) if self.native is not None and self.n > 0 else float("nan")

    @property
    def n_distinct(self) -> int:
        return int(self.totals[1])

    @property
    def n_clusters(self) -> int:
        return int(self.totals[2])

    @property
    def representatives(self) -> np.ndarray:
        """the indices of the cluster representatives, increasing; empty without clustering"""
        return np.flatnonzero(self.cluster == np.arange(self.n)).astype(np.int64)

    @property
    def consensus(self) -> np.ndarray:
        """[length] uint8: the most frequent code per position, the lowest code on ties"""
        return self.profile.argmax(axis=1).astype(np.uint8)

    @property
    def position_entropy(self) -> np.ndarray:
        """[length] float64, bits: -sum f log2 f over the codes that occur, f = count / N; NaN when N = 0"""
        if self.n == 0:
            return np.full(self.length, np.nan)
        f = self.profile.astype(np.float64) / float(self.n)
        with np.errstate(divide="ignore", invalid="ignore"):
            terms = np.where(self.profile > 0, f * np.log2(f), 0.0)
        return -terms.sum(axis=1) + 0.0

    @property
    def native_count(self) -> np.ndarray:
        """[length] int32: how many sequences hold the native's code at each position"""
        if self.native is None:
            return np.zeros(self.length, np.int32)
        return self.profile[np.arange(self.length), self.native.astype(np.int64)]

    @property
    def native_recovery(self) -> np.ndarray:
        if self.native is None or self.n == 0:
            return np.full(self.length, np.nan)
        return self.native_count.astype(np.float64) / float(self.n)


def _as_codes(item) -> np.ndarray:
    if isinstance(item, np.ndarray) and item.dtype == np.uint8 and item.ndim == 2:
        return item
    return encode(list(item))


def analyse(sets: Sequence, natives: Optional[Sequence] = None, cluster_identity: Optional[float] = 0.9, matrix: bool = False, device: int = 0,
            budget_bytes: int = batching.BATCH_BYTES, stats: Optional[dict] = None) -> List[SetResult]:
    """One ``SetResult`` per set.  A set is a list of strings or a uint8 [N, L] array of codes (an empty list is refused: it has no
    length; an array [0, L] is a set without sequences); ``natives`` holds per set a string, a uint8 [L] array or None.
    ``cluster_identity`` None: no clustering.  Sets are cut into GPU calls under ``budget_bytes`` (``set_bytes``).  Unequal lengths
    within a set, or a native of another length, is that set's ``error`` and does not stop the others.  ``stats`` receives
    ``submissions`` and ``kernel_ms``."""
    sets = list(sets)
    natives = [None] * len(sets) if natives is None else list(natives)
    if len(natives) != len(sets):
        raise ValueError(f"{len(sets)} sets and {len(natives)} natives")
    jobs, results = [], [None] * len(sets)
    for k, (item, nat) in enumerate(zip(sets, natives)):
        try:
            codes = _as_codes(item)
            if codes.shape[1] < 1:
                raise ValueError("a set needs sequences of at least one residue")
            if nat is not None:
                nat = nat if isinstance(nat, np.ndarray) and nat.dtype == np.uint8 else encode([nat])[0]
                if nat.shape != (codes.shape[1],):
                    raise ValueError(f"the native has {nat.size} residues, the sequences {codes.shape[1]}")
        except ValueError as e:
            results[k] = SetResult(f"{type(e).__name__}: {e}")
            continue
        jobs.append((k, codes, nat))

    def submit(part, timing):
        offsets = np.zeros(len(part) + 1, np.int64)
        np.cumsum([c.shape[0] for _, c, _ in part], out=offsets[1:])
        lengths = np.array([c.shape[1] for _, c, _ in part], np.int32)
        thresholds = None if cluster_identity is None else np.array([min_matches_of(cluster_identity, int(l)) for l in lengths], np.int32)
        # the native is one argument of the call: a set without one gets code 20 throughout, against which nothing is identical or known
        native = None
        if any(n is not None for _, _, n in part):
            native = np.concatenate([n if n is not None else np.full(c.shape[1], UNKNOWN, np.uint8) for _, c, n in part])
        got = seqset_arrays(np.concatenate([c.reshape(-1) for _, c, _ in part]), offsets, lengths, native, thresholds, matrix=matrix, device=device,
                            timing=timing)
        at_pos = at_matrix = 0
        for g, (k, codes, nat) in enumerate(part):
            n, length = codes.shape
            a, b = int(offsets[g]), int(offsets[g + 1])
            square = got.matrix[at_matrix:at_matrix + n * n].reshape(n, n).copy() if matrix else None
            results[k] = SetResult(None, n, length, got.seq[a:b].copy(), got.profile[at_pos:at_pos + length].copy(), got.sets[g].copy(), square, nat,
                                   -1 if thresholds is None else int(thresholds[g]),
                                   None if nat is None else ((codes < UNKNOWN) & (nat < UNKNOWN)[None, :]).sum(axis=1).astype(np.int32))
            at_pos += length
            at_matrix += n * n
    batching.run_batches(jobs, [set_bytes(c.shape[0], c.shape[1], matrix) for _, c, _ in jobs], budget_bytes, 1, submit, stats)
    return results


def identity_and_similarity(real_seq: str, predicted_seq: str, device: int = 0) -> Tuple[float, float]:
    """the reference's two numbers for one pair (ui.py): mean(a == b), and the share of positions with BLOSUM62(a, b) > 0"""
    res = analyse([[predicted_seq]], [real_seq], cluster_identity=None, device=device)[0]
    if res.error:
        raise ValueError(res.error)
    return float(res.identity_to_native[0]), float(res.similarity_to_native[0])


# ---- readers of what sample.py writes ------------------------------------------------------------------------------------------------
def read_sample_json(path) -> Dict[str, List[str]]:
    """``{key: [[sequence, ...], ...]}`` -> {key: [sequence, ...]} in file order"""
    with open(path) as f:
        data = json.load(f)
    return {str(key): [str(rec[0]) for rec in recs] for key, recs in data.items()}


def read_sample_fasta(path) -> Dict[str, List[str]]:
    """``>{key}_{n}`` records -> {key: [sequence, ...]} in file order; the key is the text before the LAST underscore.  A sequence may
    span lines."""
    out: Dict[str, List[str]] = {}
    current = None
    with open(path) as f:
        for line in f:
            line = line.strip()
            if not line:
                continue
            if line.startswith(">"):
                name = line[1:].split()[0] if line[1:].split() else ""
                key = name.rsplit("_", 1)[0] if "_" in name else name
                current = out.setdefault(key, [])
                current.append("")
            elif current is None:
                raise ValueError(f"{path}: sequence text before the first '>' line")
            else:
                current[-1] += line
    return out


def read_native_fasta(path) -> Dict[str, str]:
    """a FASTA whose names are the keys themselves -> {key: sequence}"""
    out: Dict[str, str] = {}
    key = None
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line.startswith(">"):
                key = line[1:].split()[0] if line[1:].split() else ""
                out[key] = ""
            elif line and key is not None:
                out[key] += line
    return out


def read_samples(path) -> Dict[str, List[str]]:
    """by extension: ``.json`` or anything else as FASTA"""
    return read_sample_json(path) if os.fspath(path).lower().endswith(".json") else read_sample_fasta(path)
