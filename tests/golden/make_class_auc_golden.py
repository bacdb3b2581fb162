"""Writes tests/golden/class_auc_golden.npz: scikit-learn's answers for the four matrices of
tests/class_analysis_restatement.py (GOLDEN_CASES), with the keyword arguments the reference's calculate_rotamer_metrics uses.
The matrices are not stored: the tests rebuild them with golden_matrix() and check the sha256 recorded here.

    python tests/golden/make_class_auc_golden.py            # rewrite the fixture (needs scikit-learn)
    python tests/golden/make_class_auc_golden.py --time     # time sklearn's OvO / OvR on n = 4000, k = 338 and print the host
"""
import argparse
import os
import platform
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import class_analysis_restatement as cr  # noqa: E402


def multiclass_case(name, out):
    from sklearn import metrics as sk
    x, y = cr.golden_matrix(name)
    n, k = x.shape
    labels = list(range(k))
    x64 = x.astype(np.float64)
    assert np.all(x64.sum(axis=1) == 1.0)
    own = x[np.arange(n), y]
    assert np.all((x == own[:, None]).sum(axis=1) == 1), "a true class is tied within its row"
    pred = np.argmax(x, axis=1)
    out[f"{name}_auc_ovo"] = sk.roc_auc_score(y, x64, multi_class="ovo", labels=labels, average="macro")
    try:
        ovr = sk.roc_auc_score(y, x64, multi_class="ovr", labels=labels, average="macro")
    except ValueError:
        ovr = np.nan
    out[f"{name}_auc_ovr"] = ovr
    out[f"{name}_top_k"] = np.array([sk.top_k_accuracy_score(y, x64, k=kk, labels=labels) for kk in range(1, 6)])
    out[f"{name}_precision"] = sk.precision_score(y, pred, average="macro", labels=labels, zero_division=0)
    out[f"{name}_recall"] = sk.recall_score(y, pred, average="macro", labels=labels, zero_division=0)
    cm = sk.confusion_matrix(y, pred, labels=labels)
    out[f"{name}_cm"] = cm.astype(np.int32)
    unweighted = sk.confusion_matrix(y, pred, labels=labels, normalize="all")
    count = np.bincount(y, minlength=k)
    weighted = sk.confusion_matrix(y, pred, labels=labels, normalize="all", sample_weight=count[y] / float(n))
    # sparse: the flat positions of the non-zero counts and the two normalised values there (zero elsewhere)
    nz = np.flatnonzero(cm)
    assert np.count_nonzero(unweighted) == nz.size and np.count_nonzero(weighted) == nz.size
    out[f"{name}_cm_nonzero"] = nz.astype(np.int32)
    out[f"{name}_cm_unweighted"] = unweighted.ravel()[nz]
    out[f"{name}_cm_weighted"] = weighted.ravel()[nz]


def binary_case(name, out):
    """float16 rows do not sum to 1 and sklearn's multiclass AUC refuses them: binary roc_auc_score per class (one-vs-rest) and per
    ordered pair (class a's column over the rows of class a or b), composed into the OvO macro value as sklearn composes it"""
    from sklearn import metrics as sk
    x, y = cr.golden_matrix(name)
    n, k = x.shape
    x64 = x.astype(np.float64)
    out[f"{name}_ovr_per_class"] = np.array([sk.roc_auc_score(y == c, x64[:, c]) for c in range(k)])
    present = np.unique(y)
    rows_of = {c: np.flatnonzero(y == c) for c in present}
    pair = np.full((k, k), np.nan)
    for a in present:
        for b in present:
            if a != b:
                rows = np.concatenate([rows_of[a], rows_of[b]])
                pair[a, b] = sk.roc_auc_score(y[rows] == a, x64[rows, a])
    upper = [(a, b) for i, a in enumerate(present) for b in present[i + 1:]]
    out[f"{name}_auc_ovo"] = np.mean([(pair[a, b] + pair[b, a]) / 2 for a, b in upper])
    rs = np.random.RandomState(7)
    ordered = np.array([(a, b) for a in present for b in present if a != b])
    pick = ordered[rs.choice(len(ordered), 500, replace=False)]
    out[f"{name}_pairs"] = pick.astype(np.int16)
    out[f"{name}_pair_auc"] = pair[pick[:, 0], pick[:, 1]]


def write_fixture():
    import sklearn
    out = {"sklearn_version": np.array(sklearn.__version__)}
    for name, (seed, n, k, label_classes, dtype) in cr.GOLDEN_CASES.items():
        x, y = cr.golden_matrix(name)
        out[f"{name}_seed"] = np.array(seed)
        out[f"{name}_labels"] = y
        out[f"{name}_sha256"] = np.array(cr.matrix_sha256(x))
        (binary_case if dtype == "float16" else multiclass_case)(name, out)
        print(name, {key: (float(v) if np.ndim(v) == 0 else np.shape(v)) for key, v in out.items()
                     if key.startswith(name + "_") and not key.endswith(("_sha256", "_seed"))})
    path = os.path.join(HERE, "class_auc_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


def time_sklearn():
    import sklearn
    from sklearn import metrics as sk
    rs = np.random.RandomState(1)
    n, k = 4000, 338
    z = rs.standard_normal((n, k)).astype(np.float32)
    x = np.exp(z - z.max(axis=1, keepdims=True))
    x = (x / x.sum(axis=1, keepdims=True)).astype(np.float64)
    x /= x.sum(axis=1, keepdims=True)
    y = np.concatenate([np.arange(k), rs.randint(0, k, n - k)])
    for mode in ("ovr", "ovo"):
        t0 = time.perf_counter()
        sk.roc_auc_score(y, x, multi_class=mode, labels=list(range(k)), average="macro")
        print(f"sklearn {sklearn.__version__} roc_auc_score multi_class={mode} n={n} k={k}: {time.perf_counter() - t0:.2f} s "
              f"({platform.processor() or platform.machine()}, {os.cpu_count()} CPUs, one process)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true")
    if ap.parse_args().time:
        time_sklearn()
    else:
        write_fixture()
