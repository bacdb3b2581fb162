"""NumPy restatement of th_analyse_probs (csrc/analysis.hip) and of the metrics timed_hip.analysis derives from it — the yardstick
of tests/test_analysis_host.py and tests/test_gpu_analysis.py.  Written from the definitions (include/timed_hip.h), row blocks at a
time so that a 100 k x 1024 matrix stays within a few hundred MB."""
import numpy as np

RESIDUES = "ACDEFGHIKLMNPQRSTVWY"
NEVER = 20


def restate(matrix, true_res, col_res, chunk: int = 8192):
    """(pred int8[n], rank int8[n], entropy float64[n], totals dict) for a [n, k] matrix"""
    from timed_hip.analysis import BLOSUM62
    a = np.asarray(matrix)
    n, k = a.shape
    col_res = np.asarray(col_res, dtype=np.int64)
    true_res = np.asarray(true_res, dtype=np.int64)
    owned = np.array([np.any(col_res == r) for r in range(20)])
    pred = np.empty(n, np.int8)
    rank = np.empty(n, np.int8)
    ent = np.empty(n, np.float64)
    for lo in range(0, n, chunk):
        x = a[lo:lo + chunk].astype(np.float64)
        t = true_res[lo:lo + chunk]
        m = x.shape[0]
        bad = ~np.isfinite(x).all(axis=1)
        p = col_res[np.argmax(x, axis=1)]                     # np.argmax: first maximum, first NaN
        # per residue: score = max over its columns, position = first column reaching it
        score = np.full((m, 20), -np.inf)
        first = np.full((m, 20), k, dtype=np.int64)
        for r in range(20):
            cols = np.flatnonzero(col_res == r)
            if cols.size:
                sub = x[:, cols]
                with np.errstate(invalid="ignore"):
                    score[:, r] = sub.max(axis=1)
                first[:, r] = cols[np.argmax(sub, axis=1)]
        rk = np.full(m, -1, dtype=np.int64)
        lab = t >= 0
        tt = np.where(lab, t, 0)
        st = score[np.arange(m), tt][:, None]
        ct = first[np.arange(m), tt][:, None]
        with np.errstate(invalid="ignore"):
            beats = owned[None, :] & ((score > st) | ((score == st) & (first < ct)))
        finite_rank = beats.sum(axis=1)
        finite_rank = np.where(owned[tt], finite_rank, NEVER)
        rk = np.where(lab, np.where(bad, np.where(p == t, 0, NEVER), finite_rank), -1)
        pred[lo:lo + m] = p
        rank[lo:lo + m] = rk
        # entropy in bits: H = log2 S - sum(p log2 p) / S, NaN for a zero sum, a non-finite value or a negative value
        with np.errstate(all="ignore"):
            s = x.sum(axis=1)
            plog = np.where(x > 0, x * np.log2(np.where(x > 0, x, 1.0)), 0.0).sum(axis=1)
            h = np.log2(s) - plog / s
        undefined = bad | (x < 0).any(axis=1) | ~(s > 0)
        ent[lo:lo + m] = np.where(undefined, np.nan, h)
    lab = true_res >= 0
    conf = np.zeros((20, 20), np.int64)
    np.add.at(conf, (true_res[lab], pred[lab].astype(np.int64)), 1)
    totals = {
        "confusion": conf,
        "rank_hist": np.bincount(rank[lab].astype(np.int64), minlength=21).astype(np.int64),
        "n_labelled": int(lab.sum()),
        "n_nonfinite": int(sum(int((~np.isfinite(a[lo:lo + chunk])).any(axis=1).sum()) for lo in range(0, n, chunk))),
        "n_similar": int((BLOSUM62[true_res[lab], pred[lab].astype(np.int64)] > 0).sum()),
    }
    return pred, rank, ent, totals


def metrics(true_res, pred, rank):
    """the metric values from per-row labels alone (labelled rows): top-k, macro precision / recall, confusion, bias"""
    true_res = np.asarray(true_res, dtype=np.int64)
    lab = true_res >= 0
    y, p, rk = true_res[lab], np.asarray(pred, dtype=np.int64)[lab], np.asarray(rank, dtype=np.int64)[lab]
    n = y.size
    out = {f"accuracy_{k}": float(np.mean(rk < k)) for k in range(1, 6)}
    prec, rec = [], []
    for c in range(20):
        tp = int(np.sum((y == c) & (p == c)))
        n_pred, n_true = int(np.sum(p == c)), int(np.sum(y == c))
        prec.append(tp / n_pred if n_pred else 0.0)
        rec.append(tp / n_true if n_true else 0.0)
    out["precision"], out["recall"] = float(np.mean(prec)), float(np.mean(rec))
    cm = np.zeros((20, 20))
    for a, b in zip(y, p):
        cm[a, b] += 1
    out["unweighted_cm"] = cm / n
    out["bias"] = {RESIDUES[c]: np.sum(p == c) / n - np.sum(y == c) / n for c in range(20)}
    return out
