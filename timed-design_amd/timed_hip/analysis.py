"""Evaluation of a prediction matrix against the true residues (``predict.py --output_analysis``): top-k accuracy, macro precision
and recall, the confusion matrix, per-class bias, BLOSUM62 similarity and per-residue prediction entropy — what the reference
computes with sklearn and scipy after re-reading ``<model>.csv`` (design_utils/analyse_utils.py:628-728 ``calculate_metrics``,
:294-310 ``calculate_prediction_entropy``; ui.py:55-59), here from one GPU pass over the matrix (``th_analyse_probs``,
csrc/analysis.hip) whose integer totals the functions below turn into the metrics.

Residues are indices 0..19 in the order ``RESIDUES`` (ACDEFGHIKLMNPQRSTVWY), the column order of a 20-class matrix."""
from __future__ import annotations

import ctypes as C
import typing as t

import numpy as np

from . import _lib

RESIDUES = "ACDEFGHIKLMNPQRSTVWY"
N_RES = 20

# BLOSUM62 (Henikoff & Henikoff, PNAS 89:10915, 1992), rows and columns in RESIDUES order (csrc/analysis.hip holds the same table)
BLOSUM62 = np.array([[int(v) for v in line.split()] for line in """
     4  0 -2 -1 -2  0 -2 -1 -1 -1 -1 -2 -1 -1 -1  1  0  0 -3 -2
     0  9 -3 -4 -2 -3 -3 -1 -3 -1 -1 -3 -3 -3 -3 -1 -1 -1 -2 -2
    -2 -3  6  2 -3 -1 -1 -3 -1 -4 -3  1 -1  0 -2  0 -1 -3 -4 -3
    -1 -4  2  5 -3 -2  0 -3  1 -3 -2  0 -1  2  0  0 -1 -2 -3 -2
    -2 -2 -3 -3  6 -3 -1  0 -3  0  0 -3 -4 -3 -3 -2 -2 -1  1  3
     0 -3 -1 -2 -3  6 -2 -4 -2 -4 -3  0 -2 -2 -2  0 -2 -3 -2 -3
    -2 -3 -1  0 -1 -2  8 -3 -1 -3 -2  1 -2  0  0 -1 -2 -3 -2  2
    -1 -1 -3 -3  0 -4 -3  4 -3  2  1 -3 -3 -3 -3 -2 -1  3 -3 -1
    -1 -3 -1  1 -3 -2 -1 -3  5 -2 -1  0 -1  1  2  0 -1 -2 -3 -2
    -1 -1 -4 -3  0 -4 -3  2 -2  4  2 -3 -3 -2 -2 -2 -1  1 -2 -1
    -1 -1 -3 -2  0 -3 -2  1 -1  2  5 -2 -2  0 -1 -1 -1  1 -1 -1
    -2 -3  1  0 -3  0  1 -3  0 -3 -2  6 -2  0  0  1  0 -3 -4 -2
    -1 -3 -1 -1 -4 -2 -2 -3 -1 -3 -2 -2  7 -1 -2 -1 -1 -2 -4 -3
    -1 -3  0  2 -3 -2  0 -3  1 -2  0  0 -1  5  1  0 -1 -2 -2 -1
    -1 -3 -2  0 -3 -2  0 -3  2 -2 -1  0 -2  1  5 -1 -1 -3 -3 -2
     1 -1  0  0 -2  0 -1 -2  0 -2 -1  1 -1  0 -1  4  1 -2 -3 -2
     0 -1 -1 -1 -2 -2 -2 -1 -1 -1 -1  0 -1 -1 -1  1  5  0 -2 -2
     0 -1 -3 -2 -1 -3 -3  3 -2  1  1 -3 -2 -2 -3 -2  0  4 -3 -1
    -3 -2 -4 -3  1 -2 -2 -3 -3 -2 -1 -4 -4 -2 -3 -3 -2 -3 11  2
    -2 -2 -3 -2  3 -3  2 -1 -2 -1 -1 -2 -3 -1 -2 -2 -2 -1  2  7
""".strip().splitlines()], dtype=np.int8)

_DTYPES = {np.dtype(np.float16): _lib.TH_F16, np.dtype(np.float32): _lib.TH_F32}


class Totals(C.Structure):
    """``th_analysis_totals`` of include/timed_hip.h"""
    _fields_ = [("confusion", (C.c_int64 * N_RES) * N_RES), ("rank_hist", C.c_int64 * (N_RES + 1)),
                ("n_labelled", C.c_int64), ("n_nonfinite", C.c_int64), ("n_similar", C.c_int64)]


class Analysis(t.NamedTuple):
    """What one ``th_analyse_probs`` call returns: per row the predicted residue (int8), the rank of the true residue (int8; 20 =
    never a hit, -1 = unlabelled) and the entropy in bits (float64) — each None when not requested — and the totals."""
    pred: t.Optional[np.ndarray]
    rank: t.Optional[np.ndarray]
    entropy: t.Optional[np.ndarray]
    confusion: np.ndarray          # int64 [20, 20], [true][predicted]
    rank_hist: np.ndarray          # int64 [21]
    n_labelled: int
    n_nonfinite: int
    n_similar: int


def identity_columns() -> np.ndarray:
    """col_res of a 20-class matrix"""
    return np.arange(N_RES, dtype=np.int8)


def analyse_probs(matrix, true_res, col_res, device: int = 0, rows: bool = True) -> Analysis:
    """One pass of th_analyse_probs over ``matrix`` ([n, k] float16 / float32, k <= 1024; other float types are rounded to float32)
    against ``true_res`` (n ints, 0..19 or -1) with column owners ``col_res`` (k ints, 0..19).  ``rows``: also return the per-row
    outputs.  Raises TimedHipError (code TH_EINVAL) for out-of-range arguments."""
    a = np.asarray(matrix)
    if a.ndim != 2:
        raise ValueError(f"need a 2-D [n, k] matrix, got shape {a.shape}")
    if a.dtype not in _DTYPES:
        a = a.astype(np.float32)
    a = np.ascontiguousarray(a)
    n, k = a.shape
    truth = np.ascontiguousarray(np.asarray(true_res).astype(np.int8, casting="unsafe")).reshape(-1)
    owners = np.ascontiguousarray(np.asarray(col_res).astype(np.int8, casting="unsafe")).reshape(-1)
    if truth.size != n or owners.size != k:
        raise ValueError(f"need {n} true residues and {k} column owners, got {truth.size} and {owners.size}")
    pred = np.empty(n, np.int8) if rows else None
    rank = np.empty(n, np.int8) if rows else None
    ent = np.empty(n, np.float64) if rows else None
    tot = Totals()

    def ptr(x):
        return None if x is None else x.ctypes.data_as(C.c_void_p)
    _lib.check(_lib.load().th_analyse_probs(int(device), ptr(a), _DTYPES[a.dtype], n, k, ptr(owners), ptr(truth), ptr(pred),
                                            ptr(rank), ptr(ent), C.byref(tot)))
    return Analysis(pred, rank, ent, np.ctypeslib.as_array(tot.confusion).copy(), np.ctypeslib.as_array(tot.rank_hist).copy(),
                    int(tot.n_labelled), int(tot.n_nonfinite), int(tot.n_similar))


def _ratio(a, b):
    return float(a) / float(b) if b else 0.0


def metrics_from_totals(confusion, rank_hist, n_labelled: int, n_nonfinite: int, n_similar: int, n_residues: int,
                        entropy=None) -> dict:
    """The metrics dict of ``analyse_prediction_matrix`` from the integer totals (and the per-row entropies, for mean_entropy)."""
    cm = np.asarray(confusion, dtype=np.int64).reshape(N_RES, N_RES)
    rank_hist = np.asarray(rank_hist, dtype=np.int64).reshape(N_RES + 1)
    labels, preds, tp = cm.sum(axis=1), cm.sum(axis=0), np.diag(cm)
    out: dict = {"n_residues": int(n_residues), "n_labelled": int(n_labelled), "n_nonfinite": int(n_nonfinite)}
    finite = None
    if entropy is not None:
        e = np.asarray(entropy, dtype=np.float64)
        finite = e[~np.isnan(e)]
    out["mean_entropy"] = float(finite.mean()) if finite is not None and finite.size else None
    out["count_labels"] = {c: int(v) for c, v in zip(RESIDUES, labels)}
    out["count_pred"] = {c: int(v) for c, v in zip(RESIDUES, preds)}
    out["confusion_counts"] = cm.tolist()
    out["rank_hist"] = rank_hist.tolist()
    if not n_labelled:
        for key in ("accuracy_1", "accuracy_2", "accuracy_3", "accuracy_4", "accuracy_5", "precision", "recall", "report", "bias",
                    "unweighted_cm", "similarity"):
            out[key] = None
        return out
    hits = np.cumsum(rank_hist[:N_RES])
    for kk in range(1, 6):
        out[f"accuracy_{kk}"] = float(hits[kk - 1]) / n_labelled
    precision = [_ratio(tp[c], preds[c]) for c in range(N_RES)]
    recall = [_ratio(tp[c], labels[c]) for c in range(N_RES)]
    out["precision"] = float(np.mean(precision))
    out["recall"] = float(np.mean(recall))
    out["report"] = {c: {"precision": p, "recall": r, "f1-score": (2 * p * r / (p + r) if p + r else 0.0), "support": int(s)}
                     for c, p, r, s in zip(RESIDUES, precision, recall, labels)}
    out["bias"] = {c: float(preds[i]) / n_labelled - float(labels[i]) / n_labelled for i, c in enumerate(RESIDUES)}
    out["unweighted_cm"] = (cm / float(n_labelled)).tolist()
    out["similarity"] = float(n_similar) / n_labelled
    return out


def analyse_prediction_matrix(matrix, true_res, col_res=None, device: int = 0) -> dict:
    """Accuracy, confusion and entropy of a prediction matrix ([n, k] float16 / float32; k = 20 residues, or k = 338 rotamers with
    ``col_res`` the residue of each column, e.g. from ``rotamer_columns()``) against ``true_res`` (n residue indices, -1 =
    unlabelled), computed on the GPU.  Keys follow the reference's ``calculate_metrics`` (analyse_utils.py:715-728):

    ``accuracy_1`` .. ``accuracy_5``
        the fraction of labelled rows whose true residue is among the k best residues (a residue's score is the max over its
        columns; equal scores rank by first column).  The reference's accuracy_2..5 are sklearn's top_k_accuracy_score of ONE-HOT
        predictions: every residue but the predicted one ties at 0, so they measure tie order, not the model — not comparable.
    ``precision`` / ``recall``
        macro averages over the 20 labels, standard definitions, 0 for a class never predicted (or never present).  The reference
        hands (y_pred, y_true) to sklearn in that order, so ITS "precision" is the standard recall and vice versa.
    ``report``
        per letter: precision, recall, f1-score, support (standard definitions; the reference's is transposed likewise).
    ``count_labels`` / ``count_pred``
        residue counts among the labelled rows, keyed by letter (the reference's Counters are keyed by index).
    ``bias``
        count_pred / n_labelled - count_labels / n_labelled per letter.
    ``unweighted_cm`` / ``confusion_counts``
        the [true][predicted] confusion matrix normalised by n_labelled (sklearn's normalize="all"), and its integer counts.
    ``similarity``
        the fraction of labelled rows with BLOSUM62(true, predicted) > 0 (reference ui.py:55-59).
    ``mean_entropy``
        the mean Shannon entropy in bits over every row whose entropy is defined (see th_analyse_probs; None if none is).
    ``n_residues``, ``n_labelled``, ``n_nonfinite``, ``rank_hist``
        rows, labelled rows, rows holding a NaN or an infinity, and the histogram of the true residue's rank (20 = never a hit).

    With no labelled row every metric is None."""
    a = np.asarray(matrix)
    if col_res is None:
        col_res = identity_columns()
    got = analyse_probs(a, true_res, col_res, device=device, rows=True)
    return metrics_from_totals(got.confusion, got.rank_hist, got.n_labelled, got.n_nonfinite, got.n_similar, a.shape[0], got.entropy)


def rotamer_columns(rotamers_categories) -> np.ndarray:
    """col_res of a rotamer matrix: the residue index of every category name ("ARG_1123" -> R), in column order"""
    from design_utils.amino_acids import standard_amino_acids
    one = {three: letter for letter, three in standard_amino_acids.items()}
    return np.array([RESIDUES.index(one[name.split("_")[0]]) for name in rotamers_categories], dtype=np.int8)


def residue_indices(three_letter_codes) -> np.ndarray:
    """int8 residue index of each three-letter code (ALA -> 0 ...); -1 for a code outside the 20 standard residues.  Vectorised:
    the code points of each name are packed into one integer and looked up among the 20 standard ones."""
    from design_utils.amino_acids import standard_amino_acids
    codes = np.asarray(three_letter_codes)
    if codes.dtype.kind != "U":
        codes = codes.astype(str)
    codes = np.ascontiguousarray(codes.reshape(-1))
    width = codes.dtype.itemsize // 4
    if codes.size == 0 or width < 3:
        return np.full(codes.size, -1, np.int8)
    u = codes.view(np.uint32).reshape(-1, width).astype(np.int64)
    key = (u[:, 0] << 42) | (u[:, 1] << 21) | u[:, 2]          # code points are < 2^21
    if width > 3:
        key[(u[:, 3:] != 0).any(axis=1)] = -1                 # longer names
    std = sorted((((ord(a) << 42) | (ord(b) << 21) | ord(c)), RESIDUES.index(letter))
                 for letter, (a, b, c) in standard_amino_acids.items())
    std_keys = np.array([k for k, _ in std], dtype=np.int64)
    std_index = np.array([i for _, i in std], dtype=np.int8)
    pos = np.minimum(np.searchsorted(std_keys, key), len(std_keys) - 1)
    return np.where(std_keys[pos] == key, std_index[pos], np.int8(-1)).astype(np.int8)


def entropy(matrix, device: int = 0) -> np.ndarray:
    """Shannon entropy in bits of every row (scipy.stats.entropy(row, base=2)), float64 — NaN for a row whose sum is 0 or that
    holds a NaN, an infinity or a negative value.  float16 and float32 matrices are used as they are; float64 ones are narrowed to
    float16 when that is exact (the probability CSVs predict.py writes), to float32 otherwise (values then rounded)."""
    a = np.asarray(matrix)
    if a.ndim == 1:
        a = a.reshape(1, -1)
    if a.dtype not in _DTYPES:
        a64 = a.astype(np.float64)
        with np.errstate(over="ignore", invalid="ignore"):
            h = a64.astype(np.float16)
        same = np.array_equal(h.astype(np.float64), a64, equal_nan=True)
        a = h if same else a64.astype(np.float32)
    n, k = a.shape
    if n == 0:
        return np.empty(0, np.float64)
    return analyse_probs(a, np.full(n, -1, np.int8), np.zeros(k, np.int8), device=device).entropy
