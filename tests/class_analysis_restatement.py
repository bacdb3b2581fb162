"""NumPy restatement of th_analyse_classes (csrc/class_analysis.hip) — the integer yardstick of tests/test_class_analysis_host.py and
tests/test_gpu_class_analysis.py — and the builder of the matrices behind tests/golden/class_auc_golden.npz.  Written from the
definitions in include/timed_hip.h, independently of the kernel: per column a sort of the class's own scores and two searchsorted
calls per row; arg-max by np.argmax, ranks by comparing a block of rows with its true-class column."""
import hashlib

import numpy as np


def restate(matrix, true_class, auc: bool = True, chunk: int = 4096) -> dict:
    """every integer output of th_analyse_classes for a [n, k] matrix: pred, rank (int16[n]), confusion, rank_hist, scored_count,
    pair_u2 (int64; None without ``auc``), n_labelled, n_nonfinite, n_scored"""
    a = np.asarray(matrix)
    n, k = a.shape
    t = np.asarray(true_class, dtype=np.int64).reshape(-1)
    assert t.size == n and (n == 0 or (t.min() >= -1 and t.max() < k))
    lab = t >= 0
    pred = np.zeros(n, np.int64)
    rank = np.full(n, -1, np.int64)
    finite = np.ones(n, bool)
    cols = np.arange(k)[None, :]
    for lo in range(0, n, chunk):
        x = a[lo:lo + chunk].astype(np.float64)                 # exact for float16 and float32
        tt = t[lo:lo + chunk]
        m = x.shape[0]
        finite[lo:lo + m] = np.isfinite(x).all(axis=1)
        pred[lo:lo + m] = np.argmax(x, axis=1)                  # np.argmax: first maximum, first NaN
        own = x[np.arange(m), np.where(tt >= 0, tt, 0)][:, None]
        with np.errstate(invalid="ignore"):
            above = ((x > own) | ((x == own) & (cols < tt[:, None]))).sum(axis=1)
        rank[lo:lo + m] = above
    bad = ~finite
    rank = np.where(bad, np.where(pred == t, 0, k), rank)
    rank = np.where(lab, rank, -1)
    conf = np.zeros((k, k), np.int64)
    np.add.at(conf, (t[lab], pred[lab]), 1)
    scored = lab & finite
    ts = t[scored]
    out = {
        "pred": pred.astype(np.int16), "rank": rank.astype(np.int16), "confusion": conf,
        "rank_hist": np.bincount(rank[lab], minlength=k + 1).astype(np.int64),
        "scored_count": np.bincount(ts, minlength=k).astype(np.int64),
        "pair_u2": None, "n_labelled": int(lab.sum()), "n_nonfinite": int(bad.sum()), "n_scored": int(scored.sum()),
    }
    if auc:
        u2 = np.zeros((k, k), np.int64)
        xs = a[scored]
        for c in range(k):
            col = xs[:, c].astype(np.float64) + 0.0             # -0.0 + 0.0 = +0.0
            pos = np.sort(col[ts == c])
            if pos.size == 0:
                continue
            below = np.searchsorted(pos, col, side="left").astype(np.int64)
            below_or_equal = np.searchsorted(pos, col, side="right").astype(np.int64)
            np.add.at(u2[c], ts, 2 * pos.size - below - below_or_equal)   # 2 * greater + equal
            u2[c, c] = 0
        out["pair_u2"] = u2
    return out


# ---- the matrices of the sklearn fixture, rebuilt by exact arithmetic from the frozen legacy stream -------------------------------
GOLDEN_CASES = {
    # name: (seed, n, k, labels drawn from 0..label_classes-1, dtype)
    "a": (20261, 3000, 20, 20, "float32"),
    "b": (20262, 1000, 338, 338, "float32"),
    "c": (20263, 900, 338, 200, "float32"),
    "d": (20264, 1200, 338, 338, "float16"),
}
MASS = 1 << 24


def golden_matrix(name):
    """(matrix [n, k], labels int16[n]) of fixture case ``name``: per row k non-negative integers summing to 2^24 (sorted random
    cut points, plus a random share of extra mass on the true class), divided by 2^24 in float32 — every entry and the float64 row
    sum are exact.  A row is redrawn until the true class's value is unique within it; the last n // 20 rows are copies of earlier
    rows under another label whose value is unique in that row, so that columns hold exact ties between rows."""
    seed, n, k, label_classes, dtype = GOLDEN_CASES[name]
    rs = np.random.RandomState(seed)
    n_dup = n // 20
    n_base = n - n_dup
    counts = np.zeros((n, k), np.int64)
    labels = np.zeros(n, np.int64)
    # every class at least once (when n allows), the rest drawn
    labels[:n_base] = rs.randint(0, label_classes, n_base)
    if n_base >= label_classes:
        labels[:label_classes] = rs.permutation(label_classes)
    for i in range(n_base):
        while True:
            extra = int(rs.randint(0, 8 * MASS // k))
            cuts = np.sort(rs.randint(0, MASS - extra + 1, k - 1))
            parts = np.diff(np.concatenate(([0], cuts, [MASS - extra])))
            parts[labels[i]] += extra
            if np.count_nonzero(parts == parts[labels[i]]) == 1:
                break
        counts[i] = parts
    for i in range(n_base, n):
        src = int(rs.randint(0, n_base))
        row = counts[src]
        values, inverse, freq = np.unique(row, return_inverse=True, return_counts=True)
        unique = freq[inverse] == 1
        candidates = np.flatnonzero(unique[:label_classes] & (np.arange(label_classes) != labels[src]))
        labels[i] = candidates[rs.randint(0, candidates.size)]
        counts[i] = row
    assert (counts.sum(axis=1) == MASS).all()
    x = counts.astype(np.float32) / np.float32(MASS)
    return x.astype(np.dtype(dtype)), labels.astype(np.int16)


def matrix_sha256(x) -> str:
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()
