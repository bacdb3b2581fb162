"""NumPy restatement of th_tmscore (include/timed_hip.h): the TM-score of position-paired coordinate lists as the maximum, over a
fixed schedule of seeds and a short fixed-point iteration of fits per seed, of sum 1 / (1 + (d_i / d0)^2) / L — one pair at a time,
the dtype a parameter (np.float64, or np.longdouble for the yardstick the GPU's scores are measured with).  Built on the fit, the
distances and the sequential sum of tests/superpose_restatement.py.  Computed by this file, NOT by Zhang & Skolnick's TMscore
program: the rule is this project's own reading of the published definition and search (PARITY UNPINNED AGAINST THE TM-score
PROGRAM)."""
import os

import numpy as np

import superpose_restatement as sr

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "tmscore_golden.npz")
ROUNDS = 20
MAX_POSITIONS = 4096
WIDENINGS = 4096                   # TH_TM_MAX_WIDENINGS: a selection is widened by 0.5 Angstrom at most so often
SIZES = (0, 1, 2, 3, 4, 7, 8, 21, 63, 64, 65, 76, 129)
RAGGED_SEED = 0


def d0_of(L, dtype=np.float64):
    """th_tm_d0 in ``dtype``"""
    if L <= 15:
        return dtype(0.5)
    return max(dtype(0.5), dtype(1.24) * np.cbrt(dtype(L - 15)) - dtype(1.8))


def windows(m):
    """the window lengths of the seeds: m, then halved for as long as the halved value is >= 4"""
    if m <= 0:
        return []
    out = [m]
    while out[-1] // 2 >= 4:
        out.append(out[-1] // 2)
    return out


def n_seeds_of(m):
    return sum(m - W + 1 for W in windows(m))


def seeds(m):
    """[(W, s)] in the order of the rule"""
    return [(W, s) for W in windows(m) for s in range(m - W + 1)]


def score_of(d, d0, L, dtype):
    """the SCORE of the distances of the valid positions, summed in index order"""
    q = d / d0
    return sr.seq_sum(dtype(1) / (dtype(1) + q * q)) / dtype(L)


def restate(ref, mob, norm_len=None, rounds=ROUNDS, dtype=np.float64):
    """The rule of th_tmscore on one pair.  Returns a dict: ``tm``, ``d0`` (dtype), ``counts`` [4] int64 (n_valid, L, n_seeds, n_fits),
    ``dist`` [n] dtype, ``transform`` [12] dtype, ``seed`` and ``round`` of the winner, and two figures for the tests' condition on
    their inputs: ``edge``, the smallest |d_i - cut| over every selection made, and ``gap``, the smallest relative gap between the
    two largest eigenvalues of Horn's matrix over the fits of three positions or more."""
    with np.errstate(invalid="ignore"):
        ref = np.asarray(ref, dtype=np.float64).reshape(-1, 3).astype(dtype)
        mob = np.asarray(mob, dtype=np.float64).reshape(-1, 3).astype(dtype)
    assert ref.shape == mob.shape and rounds >= 0
    n = len(ref)
    L = n if norm_len is None else int(norm_len)
    assert L >= n
    valid = np.isfinite(ref).all(axis=1) & np.isfinite(mob).all(axis=1)
    where = np.nonzero(valid)[0]
    m = len(where)
    d0 = d0_of(L, dtype)
    d_search = min(max(d0, dtype(4.5)), dtype(8.0))
    out = dict(tm=dtype(np.nan), d0=d0, counts=np.array([m, L, 0, 0], np.int64), dist=np.full(n, np.nan, dtype=dtype),
               transform=np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=dtype), seed=-1, round=-1, edge=np.inf, gap=np.inf)
    if m == 0:
        return out
    cref, cmob = ref[where], mob[where]                                        # the valid positions, compacted in index order
    everything = np.ones(m, bool)
    need = min(3, m)
    best, kept, edge, gap, n_fits = -np.inf, None, np.inf, np.inf, 0
    for number, (W, s) in enumerate(seeds(m)):
        current = np.zeros(m, bool)
        current[s:s + W] = True
        for r in range(rounds + 1):
            cm, cr, R, g = sr.fit(cref, cmob, current, dtype)
            n_fits += 1
            if int(current.sum()) >= 3:
                gap = min(gap, g)
            d = sr.distances(cref, cmob, everything, cm, cr, R, dtype)
            score = score_of(d, d0, L, dtype)
            if score > best:
                best, kept = score, (number, r, cm, cr, R, d)
            if r == rounds:
                break
            cut = d_search - dtype(1) if r == 0 else d_search + dtype(1)
            widened = 0
            while True:
                edge = min(edge, float(np.abs(d - cut).min()))
                chosen = d < cut
                if int(chosen.sum()) >= need or widened == WIDENINGS:
                    break
                cut = cut + dtype(0.5)
                widened += 1
            if int(chosen.sum()) < need or np.array_equal(chosen, current):
                break
            current = chosen
    number, r, cm, cr, R, d = kept
    out["tm"], out["seed"], out["round"] = best, number, r
    out["counts"] = np.array([m, L, n_seeds_of(m), n_fits], np.int64)
    out["dist"][where] = d
    shift = [cr[x] - ((R[x][0] * cm[0] + R[x][1] * cm[1]) + R[x][2] * cm[2]) for x in range(3)]
    out["transform"] = np.array([v for x in range(3) for v in (R[x][0], R[x][1], R[x][2], shift[x])], dtype=dtype)
    out["edge"], out["gap"] = edge, gap
    return out


def global_fit_score(ref, mob, norm_len=None, dtype=np.float64):
    """the SCORE under the one least-squares fit over every valid position: what th_superpose's cycle-0 fit gives"""
    with np.errstate(invalid="ignore"):
        ref = np.asarray(ref, dtype=np.float64).reshape(-1, 3).astype(dtype)
        mob = np.asarray(mob, dtype=np.float64).reshape(-1, 3).astype(dtype)
    L = len(ref) if norm_len is None else int(norm_len)
    valid = np.isfinite(ref).all(axis=1) & np.isfinite(mob).all(axis=1)
    if not valid.any():
        return dtype(np.nan)
    cm, cr, R, _ = sr.fit(ref, mob, valid, dtype)
    return score_of(sr.distances(ref, mob, valid, cm, cr, R, dtype)[valid], d0_of(L, dtype), L, dtype)


def score_of_distances(dist, norm_len, dtype=np.longdouble):
    """the SCORE of a list of distances (NaN: not a valid position) normalised by ``norm_len``"""
    d = np.asarray(dist, dtype=dtype)
    d = d[~np.isnan(d)]
    return score_of(d, d0_of(norm_len, dtype), norm_len, dtype) if len(d) else dtype(np.nan)


def golden_arrays(cases=None):
    """what tests/golden/tmscore_golden.npz holds: the float64 restatement's tm, d0, counts, winner, edge and gap of every 1ubq
    case, the score of the global fit, and the sha256 of the inputs"""
    cases = cases or sr.ubq_cases()
    out = {"sha256": np.array(sr.inputs_sha256(cases)), "cases": np.array(sr.CASES)}
    for name in sr.CASES:
        res = restate(*cases[name])
        out[f"{name}_tm"] = np.float64(res["tm"])
        out[f"{name}_d0"] = np.float64(res["d0"])
        out[f"{name}_counts"] = res["counts"]
        out[f"{name}_winner"] = np.array([res["seed"], res["round"]], np.int64)
        out[f"{name}_edge_gap"] = np.array([res["edge"], res["gap"]], np.float64)
        out[f"{name}_tm_global_fit"] = np.float64(global_fit_score(*cases[name]))
    return out


def ragged_batch(seed=RAGGED_SEED, copies=3):
    """every size of SIZES ``copies`` times with its own noise, in shuffled order -> [(ref, mob)]"""
    rng = np.random.default_rng(seed)
    pairs = [sr.synthetic_pair(n, rng) for n in SIZES for _ in range(copies)]
    return [pairs[k] for k in rng.permutation(len(pairs))]


def long_chain(n=MAX_POSITIONS, hinge=1000, seed=3):
    """a random walk of n positions, a rigid copy of it in another frame, and a copy whose last ``hinge`` positions are re-oriented
    about their first -> (ref, rigid, hinged)"""
    rng = np.random.default_rng(seed)
    ref, _ = sr.synthetic_pair(n, rng, outliers=False)
    rigid = ref @ sr.rotation(rng).T + rng.uniform(-30, 30, 3)
    bent = ref.copy()
    pivot = bent[n - hinge].copy()
    bent[n - hinge:] = (bent[n - hinge:] - pivot) @ sr.rotation(rng).T + pivot
    return ref, rigid, bent @ sr.rotation(rng).T + rng.uniform(-30, 30, 3)


def kabsch_transform(ref, mob):
    """(R, t) of the best proper rotation of mob onto ref by np.linalg.svd, float64: independent of the quaternion route"""
    ref, mob = np.asarray(ref, np.float64), np.asarray(mob, np.float64)
    cm, cr = mob.mean(axis=0), ref.mean(axis=0)
    U, _, Vt = np.linalg.svd((mob - cm).T @ (ref - cr))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt)) or 1.0])
    R = (U @ D @ Vt).T
    return R, cr - R @ cm


def applied_distances(ref, mob, R, t):
    """|R mob + t - ref| per position in long double"""
    ld = np.longdouble
    delta = np.asarray(mob, ld) @ np.asarray(R, ld).T + np.asarray(t, ld) - np.asarray(ref, ld)
    return np.sqrt((delta * delta).sum(axis=1))
