"""NumPy restatement of th_cealign (include/timed_hip.h): the CE structural alignment (Shindyalov & Bourne 1998) of two coordinate lists
of independent length, one pair at a time, the dtype a parameter (np.float64, or np.longdouble for the yardstick the GPU's RMSD is
measured with).  Computed by this file, NOT by the kernel and NOT by PyMOL: the rule is this project's own (PARITY UNPINNED AGAINST
PYMOL).  Every sum runs in the order the header fixes; the paths of all starts advance in lockstep, which changes no number.

restate() also reports the smallest MARGIN of every decision it makes — S against d0, c and the step score against d1, the best c
against the second best, the candidate order at rank keep / keep + 1, the winner's RMSD against the runner-up's — so that a test can
assert that its inputs put no decision on an edge before it asks a GPU for the same integers."""
import hashlib
import os

import numpy as np

import superpose_restatement as sr

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "cealign_golden.npz")
WINDOW, KEEP, MAX_POSITIONS = 8, 20, 2048
D0, D1, GAP_MAX = 3.0, 4.0, 30
S_PAIRS = [(p, q) for p in range(WINDOW) for q in range(p + 2, WINDOW)]                      # the 21 of rule 4, lexicographic
D_TERMS = [(0, 0), (7, 7)] + [(k, 7 - k) for k in range(1, 7)]                                # the 8 of rule 6, in its order
CASES = ("rigid", "noise", "hinge", "mirror", "deletion", "insertion", "helix_strand")
NOISY = ("noise", "hinge", "deletion", "insertion")
MARGINS = ("S_d0", "c_d1", "score_d1", "c_rival", "rank", "rmsd_rival")


def distance_matrix(x, dtype):
    d = x[:, None, :] - x[None, :, :]
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(dtype)


def similarity(dA, dB, mA, mB, dtype):
    """S(a, b) of every window start pair: [mA - 7, mB - 7]"""
    na, nb = mA - WINDOW + 1, mB - WINDOW + 1
    a, b = np.arange(na), np.arange(nb)
    total = None
    for p, q in S_PAIRS:
        term = np.abs(dA[a + p, a + q][:, None] - dB[b + p, b + q][None, :])
        total = term if total is None else total + term
    return total / dtype(len(S_PAIRS))


def fragment_distance(dA, dB, ai, bi, aj, bj, dtype):
    """D((ai, bi), (aj, bj)) of rule 6, broadcasting"""
    total = None
    for u, v in D_TERMS:
        term = np.abs(dA[ai + u, aj + v] - dB[bi + u, bj + v])
        total = term if total is None else total + term
    return total / dtype(WINDOW)


def candidates_of(gap_max):
    """(da, db) of g = 0 .. 2 gap_max, beyond (a + 8, b + 8)"""
    g = np.arange(2 * gap_max + 1)
    return np.where(g % 2 == 1, (g + 1) // 2, 0), np.where((g % 2 == 0) & (g > 0), g // 2, 0)


def _closest(margin, values, to):
    values = np.asarray(values, dtype=np.float64).ravel()
    return min(margin, float(np.abs(values - float(to)).min())) if values.size else margin


def trace_paths(dA, dB, S, d0, d1, gap_max, dtype, margins):
    """Rule 7 from every start at once.  -> (starts [n, 2], paths: list per start of [(a, b)], sumS, sumD)"""
    na, nb = S.shape
    starts = np.argwhere(S < d0)                                                              # row-major: ascending start index
    n_starts = len(starts)
    paths = [[(int(a), int(b))] for a, b in starts]
    sumS = S[starts[:, 0], starts[:, 1]].astype(dtype) if n_starts else np.zeros(0, dtype)
    sumD = np.zeros(n_starts, dtype)
    history = [starts.copy()] if n_starts else []                                             # history[k][row of `alive`]: AFP k
    alive = np.arange(n_starts)
    da, db = candidates_of(gap_max)
    n = 1
    while len(alive):
        last = history[-1]
        ca, cb = last[:, 0:1] + WINDOW + da[None, :], last[:, 1:2] + WINDOW + db[None, :]
        inside = (ca < na) & (cb < nb)
        sa, sb = np.where(inside, ca, 0), np.where(inside, cb, 0)
        Sc = S[sa, sb]
        ok = inside & (Sc < d0)
        s = None
        for k in range(n):
            D = fragment_distance(dA, dB, history[k][:, 0:1], history[k][:, 1:2], sa, sb, dtype)
            s = D if s is None else s + D
        c = s / dtype(n)
        margins["c_d1"] = _closest(margins["c_d1"], c[ok], d1)
        eligible = ok & (c < d1)
        cost = np.where(eligible, c, np.inf)
        g = np.argmin(cost, axis=1)                                                           # the first of equal minima: the smallest g
        rows = np.arange(len(alive))
        found = eligible[rows, g]
        if found.any() and cost.shape[1] > 1:
            ordered = np.sort(cost[found], axis=1)
            rival = (ordered[:, 1] - ordered[:, 0]).astype(np.float64)
            margins["c_rival"] = min(margins["c_rival"], float(rival.min()))
        Sg, sg = Sc[rows, g], s[rows, g]
        score = ((sumS[alive] + Sg) + (sumD[alive] + sg)) / dtype((n + 1) + (n + 1) * n // 2)
        margins["score_d1"] = _closest(margins["score_d1"], score[found], d1)
        grow = found & (score < d1)
        keep = np.nonzero(grow)[0]
        for r in keep:
            paths[alive[r]].append((int(sa[r, g[r]]), int(sb[r, g[r]])))
        sumS[alive[keep]] = sumS[alive[keep]] + Sg[keep]
        sumD[alive[keep]] = sumD[alive[keep]] + sg[keep]
        history = [h[keep] for h in history] + [np.stack([sa[keep, g[keep]], sb[keep, g[keep]]], axis=1)]
        alive = alive[keep]
        n += 1
    return starts, paths, sumS, sumD


def aligned_rmsd(A, B, path, dtype):
    """rule 9 for one path: the fit of th_superpose over its 8 n position pairs in path order -> (rmsd, cm, cr, R)"""
    ia = np.concatenate([np.arange(a, a + WINDOW) for a, _ in path])
    ib = np.concatenate([np.arange(b, b + WINDOW) for _, b in path])
    ref, mob = A[ia], B[ib]
    everything = np.ones(len(ref), bool)
    cm, cr, R, _ = sr.fit(ref, mob, everything, dtype)
    d = sr.distances(ref, mob, everything, cm, cr, R, dtype)
    return np.sqrt(sr.seq_sum(d * d) / dtype(len(d))), cm, cr, R


def restate(ref, mob, d0=D0, d1=D1, gap_max=GAP_MAX, dtype=np.float64, keep=KEEP):
    """The rule of th_cealign on one pair (ref [nA, 3], mob [nB, 3]).  Returns a dict: ``align`` int32 [nA], ``counts`` int64 [6]
    (mA, mB, n_starts, n_afps, n_aligned, n_candidates), ``rmsd`` and ``score`` of dtype, ``transform`` [12] dtype, ``path`` (the
    winner's AFPs in compacted indices), ``candidate_rmsd`` and ``margins`` {name: smallest distance to a rival or threshold}."""
    with np.errstate(invalid="ignore"):
        ref = np.asarray(ref, dtype=np.float64).reshape(-1, 3)
        mob = np.asarray(mob, dtype=np.float64).reshape(-1, 3)
    okA, okB = np.isfinite(ref).all(axis=1), np.isfinite(mob).all(axis=1)
    origA, origB = np.nonzero(okA)[0], np.nonzero(okB)[0]
    A, B = ref[okA].astype(dtype), mob[okB].astype(dtype)
    mA, mB = len(A), len(B)
    nan = dtype(np.nan)
    margins = {name: np.inf for name in MARGINS}
    out = dict(align=np.full(len(ref), -1, np.int32), counts=np.array([mA, mB, 0, 0, 0, 0], np.int64), rmsd=nan, score=nan,
               transform=np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=dtype), path=[], candidate_rmsd=[], margins=margins)
    if mA < WINDOW or mB < WINDOW:
        return out
    d0, d1 = dtype(d0), dtype(d1)
    dA, dB = distance_matrix(A, dtype), distance_matrix(B, dtype)
    S = similarity(dA, dB, mA, mB, dtype)
    margins["S_d0"] = _closest(margins["S_d0"], S, d0)
    starts, paths, sumS, sumD = trace_paths(dA, dB, S, d0, d1, int(gap_max), dtype, margins)
    n_starts = len(starts)
    if n_starts == 0:
        return out
    length = np.array([len(p) for p in paths])
    score = (sumS + sumD) / (length + length * (length - 1) // 2).astype(dtype)
    order = np.lexsort((np.arange(n_starts), score, -length))                                  # length descending, score ascending, start index
    n_cand = min(int(keep), n_starts)
    if n_starts > n_cand and length[order[n_cand - 1]] == length[order[n_cand]]:
        margins["rank"] = float(abs(score[order[n_cand]] - score[order[n_cand - 1]]))
    fits = [aligned_rmsd(A, B, paths[k], dtype) for k in order[:n_cand]]
    rmsds = [f[0] for f in fits]
    win = 0
    for k in range(1, n_cand):
        if rmsds[k] < rmsds[win]:
            win = k
    if n_cand > 1:
        margins["rmsd_rival"] = float(min(abs(rmsds[k] - rmsds[win]) for k in range(n_cand) if k != win))
    path = paths[order[win]]
    rmsd, cm, cr, R = fits[win]
    for a, b in path:
        out["align"][origA[a:a + WINDOW]] = origB[b:b + WINDOW]
    shift = [cr[x] - ((R[x][0] * cm[0] + R[x][1] * cm[1]) + R[x][2] * cm[2]) for x in range(3)]
    out.update(counts=np.array([mA, mB, n_starts, len(path), WINDOW * len(path), n_cand], np.int64), rmsd=rmsd, score=score[order[win]],
               transform=np.array([v for x in range(3) for v in (R[x][0], R[x][1], R[x][2], shift[x])], dtype=dtype), path=path,
               candidate_rmsd=rmsds)
    return out


def smallest_margin(res):
    return min(res["margins"].values())


def applied_rmsd(ref, mob, align, transform):
    """the RMSD, in long double, of the aligned positions under ``transform`` ([3, 4] or [12]): moved = R mob + t"""
    LD = np.longdouble
    T = np.asarray(transform, dtype=LD).reshape(3, 4)
    at = np.nonzero(np.asarray(align) >= 0)[0]
    a, b = np.asarray(ref, np.float64)[at].astype(LD), np.asarray(mob, np.float64)[np.asarray(align)[at]].astype(LD)
    moved = np.stack([(T[x, 0] * b[:, 0] + T[x, 1] * b[:, 1]) + T[x, 2] * b[:, 2] + T[x, 3] for x in range(3)], axis=1)
    return np.sqrt(((moved - a) ** 2).sum(axis=1).sum() / LD(len(at)))


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
CASE_SEED = 5


def ideal_chain(n, rise, radius, turn_degrees):
    t = np.arange(n) * np.radians(turn_degrees)
    return np.stack([radius * np.cos(t), radius * np.sin(t), rise * np.arange(n)], axis=1)


def ubq_cases(seed=CASE_SEED):
    """{name: (ref, mob)}: rigid, noise, hinge and mirror are those of the superposition tests; deletion lacks residues 30 .. 35 of
    the model, insertion has a 10-residue loop after position 40 (both in another frame, with 0.2 Angstrom noise); helix_strand is an
    ideal 40-residue alpha helix against an ideal 40-residue beta strand"""
    base = sr.ubq_cases(seed)
    cases = {name: base[name] for name in ("rigid", "noise", "hinge", "mirror")}
    ca = sr.ubq_ca()
    rng = np.random.default_rng(seed + 1000)

    def placed(xyz):
        return xyz @ sr.rotation(rng).T + rng.uniform(-20, 20, 3)
    noisy = ca + rng.normal(0, 0.2, ca.shape)
    cases["deletion"] = (ca, placed(np.concatenate([noisy[:30], noisy[36:]])))
    noisy = ca + rng.normal(0, 0.2, ca.shape)
    out = noisy[40] - noisy.mean(axis=0)
    out /= np.linalg.norm(out)
    side = np.cross(out, [0.0, 0.0, 1.0])
    side /= np.linalg.norm(side)
    t = np.linspace(0.0, np.pi, 12)[1:-1]
    loop = noisy[40] + out[None, :] * (12.0 * np.sin(t))[:, None] + side[None, :] * (6.0 * (1 - np.cos(t)))[:, None] + rng.normal(0, 0.2, (10, 3))
    cases["insertion"] = (ca, placed(np.concatenate([noisy[:41], loop, noisy[41:]])))
    cases["helix_strand"] = (ideal_chain(40, 1.5, 2.3, 100.0), placed(ideal_chain(40, 3.3, 0.9, 180.0)))
    return cases


def inputs_sha256(cases):
    h = hashlib.sha256()
    for name in CASES:
        for arr in cases[name]:
            h.update(np.ascontiguousarray(arr, dtype="<f8").tobytes())
    return h.hexdigest()


def golden_arrays(cases=None):
    """what tests/golden/cealign_golden.npz holds: the float64 restatement's integer tables and RMSDs, and the sha256 of the inputs"""
    cases = cases or ubq_cases()
    out = {"sha256": np.array(inputs_sha256(cases)), "cases": np.array(CASES)}
    for name in CASES:
        res = restate(*cases[name])
        out[f"{name}_counts"] = res["counts"]
        out[f"{name}_align"] = res["align"]
        out[f"{name}_rmsd"] = np.array([res["rmsd"], res["score"]], np.float64)
    return out


SIZES = (0, 7, 8, 9, 15, 16, 17, 24, 63, 64, 65, 76, 129)
RAGGED_SEED = 0


def synthetic_pair(n_ref, n_mob, rng):
    """two pieces, n_ref and n_mob long, cut at independent offsets from one random-walk chain (3.8 Angstrom steps), the model
    with sigma = 0.3 Angstrom noise in another frame; some positions NaN"""
    n = max(n_ref, n_mob) + 6
    steps = rng.normal(size=(n, 3))
    steps *= 3.8 / np.maximum(np.linalg.norm(steps, axis=1, keepdims=True), 1e-9)
    chain = np.cumsum(steps, axis=0)
    lo_r, lo_m = int(rng.integers(0, n - n_ref + 1)), int(rng.integers(0, n - n_mob + 1))
    ref = chain[lo_r:lo_r + n_ref].copy()
    mob = (chain[lo_m:lo_m + n_mob] + rng.normal(0, 0.3, (n_mob, 3))) @ sr.rotation(rng).T + rng.uniform(-30, 30, 3)
    if n_ref >= 16 and rng.random() < 0.5:
        ref[int(rng.integers(0, n_ref)), int(rng.integers(0, 3))] = np.nan
    if n_mob >= 16 and rng.random() < 0.5:
        mob[int(rng.integers(0, n_mob)), int(rng.integers(0, 3))] = [np.nan, np.inf, -np.inf][int(rng.integers(0, 3))]
    return ref, mob


def ragged_batch(seed=RAGGED_SEED):
    """26 pairs: every size of SIZES twice as the reference, against a model of ANOTHER size of SIZES, in shuffled order"""
    rng = np.random.default_rng(seed)
    pairs = []
    for shift in (3, 8):
        for k, n in enumerate(SIZES):
            pairs.append(synthetic_pair(n, SIZES[(k + shift) % len(SIZES)], rng))
    return [pairs[k] for k in rng.permutation(len(pairs))]


LONG_POSITIONS, LONG_D0, LONG_GAP_MAX = 560, 0.6, 2


def long_pair(seed=11):
    """a random-walk chain of 560 positions against a copy in another frame, with sigma = 0.05 Angstrom noise, that lacks the first
    three residues: with d0 = 0.6 almost only the diagonal starts a path, and the 20 longest paths have 66 AFPs or more — more than
    the 64 that one register of the kernel's path holds, and more position pairs than one pass of a wavefront"""
    rng = np.random.default_rng(seed)
    steps = rng.normal(size=(LONG_POSITIONS, 3))
    steps *= 3.8 / np.linalg.norm(steps, axis=1, keepdims=True)
    ref = np.cumsum(steps, axis=0)
    mob = ref[3:] + rng.normal(0, 0.05, (LONG_POSITIONS - 3, 3))
    return ref, mob @ sr.rotation(rng).T + rng.uniform(-30, 30, 3)


def flatten(pairs):
    """(ref [ref_total, 3], ref_offsets, mob [mob_total, 3], mob_offsets) of a list of (ref, mob)"""
    def side(arrays):
        offsets = np.concatenate([[0], np.cumsum([len(a) for a in arrays])]).astype(np.int64)
        xyz = np.concatenate([np.asarray(a, np.float64).reshape(-1, 3) for a in arrays] + [np.zeros((0, 3))])
        return xyz, offsets
    ref, ro = side([r for r, _ in pairs])
    mob, mo = side([m for _, m in pairs])
    return ref, ro, mob, mo


def restate_batch(ref, ref_offsets, mob, mob_offsets, d0=D0, d1=D1, gap_max=GAP_MAX, dtype=np.float64):
    ref, mob = np.asarray(ref, np.float64).reshape(-1, 3), np.asarray(mob, np.float64).reshape(-1, 3)
    return [restate(ref[a:b], mob[c:d], d0, d1, gap_max, dtype)
            for a, b, c, d in zip(ref_offsets[:-1], ref_offsets[1:], mob_offsets[:-1], mob_offsets[1:])]
