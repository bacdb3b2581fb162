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
from ._lib import ptr

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


# ---- per-class evaluation (th_analyse_classes, csrc/class_analysis.hip): analyse_rotamers.py, predict.py --output_auc ------------
class ClassCounts(C.Structure):
    """``th_class_counts`` of include/timed_hip.h"""
    _fields_ = [("n_labelled", C.c_int64), ("n_nonfinite", C.c_int64), ("n_scored", C.c_int64)]


class ClassAnalysis(t.NamedTuple):
    """What one ``th_analyse_classes`` call returns: per row the predicted class and the rank of the true class (int16; k = a
    non-finite row that was missed, -1 = unlabelled; None when not requested), and the integer totals."""
    pred: t.Optional[np.ndarray]
    rank: t.Optional[np.ndarray]
    confusion: np.ndarray          # int64 [k, k], [true][predicted], labelled rows
    rank_hist: np.ndarray          # int64 [k + 1]
    scored_count: np.ndarray       # int64 [k]: labelled rows without NaN / infinity, per class
    pair_u2: t.Optional[np.ndarray]  # int64 [k, k]: U2[a][b], twice the Mann-Whitney statistic of column a, class a against class b
    n_labelled: int
    n_nonfinite: int
    n_scored: int


def analyse_classes(matrix, true_class, device: int = 0, auc: bool = True, rows: bool = True) -> ClassAnalysis:
    """One call of th_analyse_classes over ``matrix`` ([n, k] float16 / float32, k <= 1024; other float types are rounded to
    float32) against ``true_class`` (n ints, 0..k-1 or -1).  ``auc``: also fill ``pair_u2`` (a second sweep of the matrix);
    ``rows``: also return the per-row outputs.  Raises TimedHipError (code TH_EINVAL) for out-of-range arguments."""
    a = np.asarray(matrix)
    if a.ndim != 2:
        raise ValueError(f"need a 2-D [n, k] matrix, got shape {a.shape}")
    if a.dtype not in _DTYPES:
        a = a.astype(np.float32)
    a = np.ascontiguousarray(a)
    n, k = a.shape
    wide = np.asarray(true_class).reshape(-1)
    if wide.size != n:
        raise ValueError(f"need {n} true classes, got {wide.size}")
    if wide.size and (wide.min() < -1 or wide.max() > 32767):
        raise _lib.TimedHipError(_lib.TH_EINVAL, f"true class outside -1..{k - 1}")
    truth = np.ascontiguousarray(wide.astype(np.int16, casting="unsafe"))
    pred = np.empty(n, np.int16) if rows else None
    rank = np.empty(n, np.int16) if rows else None
    kk = max(k, 0)
    conf = np.zeros((kk, kk), np.int64)
    hist = np.zeros(kk + 1, np.int64)
    scored = np.zeros(kk, np.int64)
    u2 = np.zeros((kk, kk), np.int64) if auc else None
    cnt = ClassCounts()
    _lib.check(_lib.load().th_analyse_classes(int(device), ptr(a), _DTYPES[a.dtype], n, k, ptr(truth), ptr(pred), ptr(rank),
                                              ptr(conf), ptr(hist), ptr(scored), ptr(u2), C.byref(cnt)))
    return ClassAnalysis(pred, rank, conf, hist, scored, u2, int(cnt.n_labelled), int(cnt.n_nonfinite), int(cnt.n_scored))


def roc_auc_from_pairs(pair_u2, scored_count) -> dict:
    """ROC AUC one-vs-one and one-vs-rest (macro) from the integer table of th_analyse_classes, in float64.  With n_c =
    scored_count[c] and N their sum: auc(a|b) = U2[a][b] / (2 n_a n_b) is sklearn's binary roc_auc_score(y == a, x[:, a]) over the
    rows of class a or b.

    ``auc_ovo``            mean over unordered pairs of PRESENT classes (n_c > 0) of (auc(a|b) + auc(b|a)) / 2 — sklearn's
                           multi_class="ovo", average="macro"; None with fewer than two classes present
    ``auc_ovr_per_class``  per class c: sum_b U2[c][b] / (2 n_c (N - n_c)); None where n_c = 0 or n_c = N
    ``auc_ovr``            their mean over all k classes (multi_class="ovr", average="macro"); None if any is undefined
    ``auc_ovr_present``    their mean over the classes where it is defined; None if there is none
    ``n_classes_present``  classes with n_c > 0"""
    cnt = np.asarray(scored_count, dtype=np.int64).reshape(-1)
    k = cnt.size
    u2 = np.asarray(pair_u2, dtype=np.int64).reshape(k, k)
    present = np.flatnonzero(cnt > 0)
    total = int(cnt.sum())
    out: dict = {"n_classes_present": int(present.size)}
    if present.size >= 2:
        nf = cnt[present].astype(np.float64)
        q = u2[np.ix_(present, present)].astype(np.float64) / (2.0 * np.outer(nf, nf))
        upper = np.triu_indices(present.size, 1)
        out["auc_ovo"] = float(np.mean((q[upper] + q.T[upper]) / 2.0))
    else:
        out["auc_ovo"] = None
    row = u2.sum(axis=1)
    per = [float(row[c]) / (2.0 * float(cnt[c]) * float(total - cnt[c])) if 0 < cnt[c] < total else None for c in range(k)]
    defined = [v for v in per if v is not None]
    out["auc_ovr_per_class"] = per
    out["auc_ovr"] = float(np.mean(defined)) if k and len(defined) == k else None
    out["auc_ovr_present"] = float(np.mean(defined)) if defined else None
    return out


def weighted_confusion(confusion) -> t.Optional[np.ndarray]:
    """The reference's label-weighted confusion matrix — sklearn's confusion_matrix(sample_weight = count[y] / N,
    normalize="all") — from the integer one: cm[t][p] n_t / sum_t n_t^2.  None for an empty matrix."""
    cm = np.asarray(confusion, dtype=np.int64)
    labels = cm.sum(axis=1).astype(np.float64)
    denom = float(np.sum(labels * labels))
    return cm * labels[:, None] / denom if denom else None


def class_metrics_from_totals(confusion, rank_hist, scored_count, pair_u2, n_labelled: int, n_nonfinite: int, n_scored: int,
                              n_rows: int, categories=None) -> dict:
    """The metrics dict of ``analyse_class_matrix`` from the integer totals of th_analyse_classes; ``categories``: the k class
    names that key the per-class entries (default "0" .. "k-1")."""
    cm = np.asarray(confusion, dtype=np.int64)
    k = cm.shape[0]
    rank_hist = np.asarray(rank_hist, dtype=np.int64).reshape(k + 1)
    names = [str(c) for c in (categories if categories is not None else range(k))]
    if len(names) != k:
        raise ValueError(f"need {k} category names, got {len(names)}")
    labels, preds, tp = cm.sum(axis=1), cm.sum(axis=0), np.diag(cm)
    out: dict = {"n_rows": int(n_rows), "n_classes": int(k), "n_labelled": int(n_labelled), "n_nonfinite": int(n_nonfinite),
                 "n_scored": int(n_scored)}
    out["count_labels"] = {c: int(v) for c, v in zip(names, labels)}
    out["count_pred"] = {c: int(v) for c, v in zip(names, preds)}
    out["confusion_counts"] = cm.tolist()
    out["rank_hist"] = rank_hist.tolist()
    if pair_u2 is not None:
        out.update(roc_auc_from_pairs(pair_u2, scored_count))
    else:
        out.update({"auc_ovo": None, "auc_ovr": None, "auc_ovr_present": None, "auc_ovr_per_class": None,
                    "n_classes_present": int(np.count_nonzero(np.asarray(scored_count)))})
    if not n_labelled:
        for key in ("accuracy_1", "accuracy_2", "accuracy_3", "accuracy_4", "accuracy_5", "precision", "recall", "report", "bias",
                    "unweighted_cm", "weighted_cm"):
            out[key] = None
        return out
    hits = np.cumsum(rank_hist[:k])
    for kk in range(1, 6):
        out[f"accuracy_{kk}"] = float(hits[min(kk, k) - 1]) / n_labelled
    precision = [_ratio(tp[c], preds[c]) for c in range(k)]
    recall = [_ratio(tp[c], labels[c]) for c in range(k)]
    out["precision"] = float(np.mean(precision))
    out["recall"] = float(np.mean(recall))
    out["report"] = {c: {"precision": p, "recall": r, "f1-score": (2 * p * r / (p + r) if p + r else 0.0), "support": int(s)}
                     for c, p, r, s in zip(names, precision, recall, labels)}
    out["bias"] = {c: (float(preds[i]) / n_labelled - float(labels[i]) / n_labelled if preds[i] else None)
                   for i, c in enumerate(names)}
    out["unweighted_cm"] = (cm / float(n_labelled)).tolist()
    out["weighted_cm"] = weighted_confusion(cm).tolist()
    return out


def analyse_class_matrix(matrix, true_class, categories=None, device: int = 0) -> dict:
    """Per-class metrics of a prediction matrix ([n, k] float16 / float32, e.g. the k = 338 rotamer classes) against
    ``true_class`` (n class indices, -1 = unlabelled), computed on the GPU (``th_analyse_classes``).  Keys follow the reference's
    ``calculate_rotamer_metrics`` (analyse_utils.py:731-898); per-class entries are keyed by ``categories`` (default "0".."k-1"):

    ``auc_ovo`` / ``auc_ovr``
        ROC AUC one-vs-one and one-vs-rest, macro average: sklearn's roc_auc_score(multi_class="ovo" | "ovr", average="macro",
        labels=range(k)), from exact integer Mann-Whitney counts over the scored rows (labelled, no NaN, no infinity).  OvO
        averages over the classes present; OvR is None unless every one of the k classes has a scored row (sklearn raises or
        returns NaN there, and the reference writes NaN).  ``auc_ovr_present`` is the OvR mean over the classes where it is
        defined, ``auc_ovr_per_class`` the list (None where undefined), ``n_classes_present`` their number.
        DIFFERENCE from the reference: calculate_rotamer_metrics adds (1 - rowsum) / 338 to every entry of a row whose sum is not
        1 (float16 softmax rows never are), because sklearn refuses such rows; that shifts every row by its own amount and can
        reorder near-ties between rows.  Here the AUC is of the matrix AS STORED: no residual is spread.
    ``accuracy_1`` .. ``accuracy_5``
        the fraction of labelled rows whose true class is among the k best columns (equal values rank by lower column first;
        sklearn's top_k_accuracy_score agrees on rows whose true class is not tied).
    ``precision`` / ``recall``
        macro averages over all k labels, standard orientation, 0 for a class never predicted (or never present).
    ``report``
        per category: precision, recall, f1-score, support.
    ``count_labels`` / ``count_pred`` / ``bias``
        class counts among the labelled rows, and count_pred / n_labelled - count_labels / n_labelled; the bias of a class that is
        never predicted is None (the reference writes NaN).
    ``unweighted_cm`` / ``weighted_cm`` / ``confusion_counts``
        the [true][predicted] confusion matrix normalised by n_labelled (sklearn's normalize="all"); the same with every row
        weighted by its label's frequency (sample_weight = count[y] / N: cm[t][p] n_t / sum n_t^2); and the integer counts.
    ``n_rows``, ``n_classes``, ``n_labelled``, ``n_nonfinite``, ``n_scored``, ``rank_hist``
        rows, columns, labelled rows, rows holding a NaN or an infinity, scored rows, and the histogram of the true class's rank.

    With no labelled row every metric is None.  Entropy is not repeated here (``analyse_prediction_matrix`` has it)."""
    a = np.asarray(matrix)
    got = analyse_classes(a, true_class, device=device, auc=True, rows=False)
    return class_metrics_from_totals(got.confusion, got.rank_hist, got.scored_count, got.pair_u2, got.n_labelled, got.n_nonfinite,
                                     got.n_scored, a.shape[0], categories)
