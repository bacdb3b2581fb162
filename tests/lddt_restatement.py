"""NumPy restatement of th_lddt (include/timed_hip.h): the local Distance Difference Test of position-paired coordinate lists in the
CA-only form, one pair at a time, the dtype a parameter (np.float64, or np.longdouble to show that no decision of a test sits where
the precision matters).  Every product and sum is one NumPy operation, so each is rounded on its own; np.sqrt is correctly rounded.
Computed by this file, NOT by OpenStructure and NOT by AlphaFold's lddt.py, neither of which is available: the rule is this project's
reading of the published definition (PARITY UNPINNED AGAINST OPENSTRUCTURE).

The inputs are those of tests/superpose_restatement.py (``ubq_cases``, ``ragged_batch``, ``flatten``)."""
import os

import numpy as np

import superpose_restatement as sr

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "lddt_golden.npz")
RADIUS = 15.0
THRESHOLDS = (0.5, 1.0, 2.0, 4.0)
CASES = sr.CASES


def distances(xyz):
    """d[i, j] = sqrt((dx*dx + dy*dy) + dz*dz) in the array's dtype"""
    dx = xyz[None, :, 0] - xyz[:, None, 0]
    dy = xyz[None, :, 1] - xyz[:, None, 1]
    dz = xyz[None, :, 2] - xyz[:, None, 2]
    return np.sqrt((dx * dx + dy * dy) + dz * dz)


def restate(ref, mob, radius=RADIUS, thresholds=THRESHOLDS, dtype=np.float64):
    """The rule of th_lddt on one pair.  Returns a dict: ``residue`` [n, 5] int32 (n_i, c_i[0..3]), ``pair`` [6] int64 (n_valid, N,
    C[0..3]) and ``edge``: the smallest of |d_ref - radius| over the ordered pairs of valid positions and of ||d_ref - d_mob| - t|
    over the included pairs and the four thresholds (inf when there is no such pair) — how far the nearest decision is from its
    tie."""
    ref = np.asarray(ref, dtype=np.float64).reshape(-1, 3)
    mob = np.asarray(mob, dtype=np.float64).reshape(-1, 3)
    assert ref.shape == mob.shape and len(thresholds) == 4
    n = len(ref)
    valid = np.isfinite(ref).all(axis=1) & np.isfinite(mob).all(axis=1)
    residue = np.zeros((n, 5), np.int32)
    edge = np.inf
    idx = np.nonzero(valid)[0]
    if len(idx) > 1:
        with np.errstate(over="ignore", invalid="ignore"):
            d_ref = distances(ref[idx].astype(dtype))
            d_mob = distances(mob[idx].astype(dtype))
            other = ~np.eye(len(idx), dtype=bool)
            included = other & (d_ref < dtype(radius))
            diff = np.abs(d_ref - d_mob)
            edge = min(edge, float(np.abs(d_ref - dtype(radius))[other].min()))
            residue[idx, 0] = included.sum(axis=1)
            for k, t in enumerate(thresholds):
                residue[idx, 1 + k] = (included & (diff < dtype(t))).sum(axis=1)
                if included.any():
                    edge = min(edge, float(np.abs(diff - dtype(t))[included].min()))
    pair = np.concatenate([[int(valid.sum())], residue.astype(np.int64).sum(axis=0)]).astype(np.int64)
    return dict(residue=residue, pair=pair, edge=edge)


def restate_batch(ref, mob, offsets, radius=RADIUS, thresholds=THRESHOLDS, dtype=np.float64):
    """the tables th_lddt returns for a flat batch, and the smallest edge: (residue [total, 5] int32, pair [P, 6] int64, edge)"""
    ref, mob = np.asarray(ref, np.float64).reshape(-1, 3), np.asarray(mob, np.float64).reshape(-1, 3)
    offsets = np.asarray(offsets, np.int64).reshape(-1)
    parts = [restate(ref[lo:hi], mob[lo:hi], radius, thresholds, dtype) for lo, hi in zip(offsets[:-1], offsets[1:])]
    residue = np.concatenate([p["residue"] for p in parts]) if parts else np.zeros((0, 5), np.int32)
    pair = np.stack([p["pair"] for p in parts]) if parts else np.zeros((0, 6), np.int64)
    return residue, pair, min([p["edge"] for p in parts], default=np.inf)


def score(pair):
    """lddt = sum_k C[k] / (4 N) of one row of the pair table, NaN when N = 0"""
    return float(pair[2:6].sum()) / (4.0 * float(pair[1])) if pair[1] else float("nan")


def golden_arrays(cases=None):
    """what tests/golden/lddt_golden.npz holds: the float64 restatement's integer tables for every case at the default radius and
    thresholds, and the sha256 of the inputs"""
    cases = cases or sr.ubq_cases()
    out = {"sha256": np.array(sr.inputs_sha256(cases)), "cases": np.array(CASES)}
    for name in CASES:
        res = restate(*cases[name])
        out[f"{name}_residue"], out[f"{name}_pair"] = res["residue"], res["pair"]
    return out


def tie_pairs():
    """Pairs whose decisions sit EXACTLY on a tie, with exact square roots (3-4-5 and 9-12-15 triangles, halves), and the integers
    the strict inequalities give: -> ([(ref, mob)], residue [total, 5], pair [P, 6])."""
    o = [0.0, 0.0, 0.0]
    pairs, rows = [], []
    # d_ref = 15 exactly: not included, whatever the model does
    pairs.append((np.array([o, [9.0, 12.0, 0.0]]), np.array([o, [9.0, 12.0, 0.0]])))
    rows += [[0, 0, 0, 0, 0]] * 2
    # d_ref = 5, d_mob = 5 + t and 5 - t: the difference is exactly the threshold t, which is not preserved at t itself
    for k, t in enumerate(THRESHOLDS):
        for d_mob in (5.0 + t, 5.0 - t):
            pairs.append((np.array([o, [3.0, 4.0, 0.0]]), np.array([o, [0.0, 0.0, d_mob]])))
            rows += [[1] + [1 if t < u else 0 for u in THRESHOLDS]] * 2
    # three positions: d_ref(0, 1) = 15 (excluded), d_ref(0, 2) = 5 against 5.5 (a tie at 0.5), d_ref(1, 2) = 10 against 10
    pairs.append((np.array([o, [9.0, 12.0, 0.0], [3.0, 4.0, 0.0]]), np.array([o, [11.5, 8.0, 0.0], [5.5, 0.0, 0.0]])))
    rows += [[1, 0, 1, 1, 1], [1, 1, 1, 1, 1], [2, 1, 2, 2, 2]]
    residue = np.array(rows, np.int32)
    offsets = np.concatenate([[0], np.cumsum([len(r) for r, _ in pairs])])
    pair = np.array([[hi - lo] + residue[lo:hi].astype(np.int64).sum(axis=0).tolist() for lo, hi in zip(offsets[:-1], offsets[1:])], np.int64)
    return pairs, residue, pair
