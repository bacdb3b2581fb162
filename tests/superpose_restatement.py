"""NumPy restatement of th_superpose (include/timed_hip.h): position-paired least-squares superposition with outlier-rejection
refinement, one pair at a time, the dtype a parameter (np.float64, or np.longdouble for the yardstick the GPU's distances and RMSDs
are measured with).  Sums run in index order (np.cumsum is sequential); the 4 x 4 Jacobi solver is scalar NumPy so that it runs in
long double as well.  Computed by this file, NOT by PyMOL: the rule is this project's own (PARITY UNPINNED AGAINST PYMOL).

Also an independent SVD Kabsch, the seeded cases derived from the CA atoms of tests/golden/1ubq.pdb1.gz and the synthetic chains
that tests/test_superpose_host.py and tests/test_gpu_superpose.py share."""
import gzip
import hashlib
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
UBQ = os.path.join(HERE, "golden", "1ubq.pdb1.gz")
GOLDEN = os.path.join(HERE, "golden", "superpose_golden.npz")
SWEEPS = 10
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
GDT_CUTS = (1.0, 2.0, 4.0, 8.0)
CASES = ("rigid", "noise", "hinge", "mirror", "invalid")
# The distances of a rigid copy are rounding noise (1e-14): a cutoff in units of their RMS would put every decision on an edge, so
# that case runs without refinement; the others with PyMOL's default.
CASE_CYCLES = {"rigid": 0, "noise": 5, "hinge": 5, "mirror": 5, "invalid": 5}


def seq_sum(a):
    """sum along axis 0 in index order, every partial sum rounded in the array's dtype"""
    return np.cumsum(a, axis=0)[-1]


def jacobi4(A, dtype):
    """cyclic Jacobi on a symmetric 4 x 4 matrix: (diagonal, eigenvectors in columns).  Scalars of ``dtype`` throughout."""
    one, two, zero = dtype(1), dtype(2), dtype(0)
    A = [[dtype(A[i][j]) for j in range(4)] for i in range(4)]
    V = [[one if i == j else zero for j in range(4)] for i in range(4)]
    for _ in range(SWEEPS):
        if all(A[p][q] == 0 for p, q in PAIRS):
            break
        for p, q in PAIRS:
            apq = A[p][q]
            if apq == 0:
                continue
            with np.errstate(over="ignore"):                               # a vanishing apq: theta and root infinite, t = 0
                theta = (A[q][q] - A[p][p]) / (two * apq)
                root = abs(theta) + np.sqrt(theta * theta + one)
            t = (one if theta >= 0 else -one) / root
            c = one / np.sqrt(t * t + one)
            s = t * c
            for k in range(4):
                akp, akq = A[k][p], A[k][q]
                A[k][p], A[k][q] = c * akp - s * akq, s * akp + c * akq
            for k in range(4):
                apk, aqk = A[p][k], A[q][k]
                A[p][k], A[q][k] = c * apk - s * aqk, s * apk + c * aqk
            A[p][q] = A[q][p] = zero
            for k in range(4):
                vkp, vkq = V[k][p], V[k][q]
                V[k][p], V[k][q] = c * vkp - s * vkq, s * vkp + c * vkq
    return [A[k][k] for k in range(4)], V


def horn_matrix(S):
    return [[(S[0][0] + S[1][1]) + S[2][2], S[1][2] - S[2][1], S[2][0] - S[0][2], S[0][1] - S[1][0]],
            [S[1][2] - S[2][1], (S[0][0] - S[1][1]) - S[2][2], S[0][1] + S[1][0], S[2][0] + S[0][2]],
            [S[2][0] - S[0][2], S[0][1] + S[1][0], (S[1][1] - S[0][0]) - S[2][2], S[1][2] + S[2][1]],
            [S[0][1] - S[1][0], S[2][0] + S[0][2], S[1][2] + S[2][1], (S[2][2] - S[0][0]) - S[1][1]]]


def fit(ref, mob, kept, dtype):
    """-> (cm, cr, R as nested lists, relative gap between the two largest eigenvalues of Horn's matrix)"""
    idx = np.nonzero(kept)[0]
    count = dtype(len(idx))
    cm, cr = seq_sum(mob[idx]) / count, seq_sum(ref[idx]) / count
    a, b = mob[idx] - cm, ref[idx] - cr
    S = [[seq_sum(a[:, x] * b[:, y]) for y in range(3)] for x in range(3)]
    values, V = jacobi4(horn_matrix(S), dtype)
    top = 0
    for k in range(1, 4):
        if values[k] > values[top]:
            top = k
    w, x, y, z = (V[k][top] for k in range(4))
    length = np.sqrt(((w * w + x * x) + y * y) + z * z)
    w, x, y, z = w / length, x / length, y / length, z / length
    ww, xx, yy, zz, two = w * w, x * x, y * y, z * z, dtype(2)
    R = [[((ww + xx) - yy) - zz, two * (x * y - w * z), two * (x * z + w * y)],
         [two * (x * y + w * z), ((ww - xx) + yy) - zz, two * (y * z - w * x)],
         [two * (x * z - w * y), two * (y * z + w * x), ((ww - xx) - yy) + zz]]
    ordered = sorted((float(v) for v in values), reverse=True)
    gap = (ordered[0] - ordered[1]) / abs(ordered[0]) if ordered[0] != 0 else 0.0
    return cm, cr, R, gap


def distances(ref, mob, valid, cm, cr, R, dtype):
    d = np.full(len(ref), np.nan, dtype=dtype)
    a = mob[valid] - cm
    delta = [(((R[x][0] * a[:, 0] + R[x][1] * a[:, 1]) + R[x][2] * a[:, 2]) + cr[x]) - ref[valid][:, x] for x in range(3)]
    d[valid] = np.sqrt((delta[0] * delta[0] + delta[1] * delta[1]) + delta[2] * delta[2])
    return d


def restate(ref, mob, cycles=5, cutoff=2.0, dtype=np.float64):
    """The rule of th_superpose on one pair.  Returns a dict: ``dist`` [n] dtype, ``kept`` [n] uint8, ``rmsd`` [3] dtype (kept, all,
    fit_all), ``counts`` [7] int32, ``transform`` [12] dtype, and two figures for the tests' condition on their inputs: ``edge``,
    the smallest distance of any valid d_i to 1, 2, 4, 8 (final fit) or of any kept d_i to a cycle's cutoff * rms, and ``gap``, the
    smallest relative gap between the two largest eigenvalues of Horn's matrix over the fits made."""
    with np.errstate(invalid="ignore"):
        ref = np.asarray(ref, dtype=np.float64).reshape(-1, 3).astype(dtype)
        mob = np.asarray(mob, dtype=np.float64).reshape(-1, 3).astype(dtype)
    assert ref.shape == mob.shape
    n = len(ref)
    valid = np.isfinite(ref).all(axis=1) & np.isfinite(mob).all(axis=1)
    n_valid = int(valid.sum())
    nan = dtype(np.nan)
    out = dict(dist=np.full(n, np.nan, dtype=dtype), kept=valid.astype(np.uint8), rmsd=np.array([nan, nan, nan], dtype=dtype),
               counts=np.zeros(7, np.int32), transform=np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=dtype), edge=np.inf, gap=np.inf)
    if n_valid == 0:
        return out
    kept = valid.copy()
    cycles_run, edge, gap, fit_all = 0, np.inf, np.inf, nan
    while True:
        cm, cr, R, g = fit(ref, mob, kept, dtype)
        gap = min(gap, g)
        d = distances(ref, mob, valid, cm, cr, R, dtype)
        n_kept = int(kept.sum())
        rms = np.sqrt(seq_sum(d[kept] * d[kept]) / dtype(n_kept))
        if cycles_run == 0:
            fit_all = rms
        if cycles_run >= cycles or n_valid < 3:
            break
        limit = dtype(cutoff) * rms
        edge = min(edge, float(np.abs(d[kept] - limit).min()))
        drop = kept & (np.nan_to_num(d, nan=-1.0) > limit)
        if not drop.any() or n_kept - int(drop.sum()) < 3:
            break
        kept &= ~drop
        cycles_run += 1
    dv = d[valid]
    for cut in GDT_CUTS:
        edge = min(edge, float(np.abs(dv - dtype(cut)).min()))
    out["dist"], out["kept"] = d, kept.astype(np.uint8)
    out["rmsd"] = np.array([rms, np.sqrt(seq_sum(dv * dv) / dtype(n_valid)), fit_all], dtype=dtype)
    out["counts"] = np.array([n_valid, int(kept.sum()), cycles_run] + [int((dv <= dtype(cut)).sum()) for cut in GDT_CUTS], np.int32)
    shift = [cr[x] - ((R[x][0] * cm[0] + R[x][1] * cm[1]) + R[x][2] * cm[2]) for x in range(3)]
    out["transform"] = np.array([v for x in range(3) for v in (R[x][0], R[x][1], R[x][2], shift[x])], dtype=dtype)
    out["edge"], out["gap"] = edge, gap
    return out


def restate_batch(ref, mob, offsets, cycles=5, cutoff=2.0, dtype=np.float64):
    """the arrays th_superpose returns for a flat batch: (dist, kept, rmsd [P, 3], counts [P, 7], transform [P, 12], edge, gap)"""
    ref, mob = np.asarray(ref, np.float64).reshape(-1, 3), np.asarray(mob, np.float64).reshape(-1, 3)
    parts = [restate(ref[lo:hi], mob[lo:hi], cycles, cutoff, dtype) for lo, hi in zip(offsets[:-1], offsets[1:])]
    cat = lambda key, shape, dt: (np.concatenate([p[key].reshape(shape) for p in parts]) if parts else np.zeros(shape, dt).reshape((0,) + shape[1:]))  # noqa: E731
    return (cat("dist", (-1,), dtype), cat("kept", (-1,), np.uint8), cat("rmsd", (1, 3), dtype), cat("counts", (1, 7), np.int32),
            cat("transform", (1, 12), dtype), min([p["edge"] for p in parts], default=np.inf), min([p["gap"] for p in parts], default=np.inf))


def kabsch_rmsd(ref, mob):
    """the conventional RMSD after the best PROPER rotation, by np.linalg.svd with the determinant correction — independent of the
    quaternion route above"""
    ref, mob = np.asarray(ref, np.float64), np.asarray(mob, np.float64)
    ok = np.isfinite(ref).all(axis=1) & np.isfinite(mob).all(axis=1)
    a, b = mob[ok] - mob[ok].mean(axis=0), ref[ok] - ref[ok].mean(axis=0)
    U, _, Vt = np.linalg.svd(a.T @ b)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt)) or 1.0])
    rot = (U @ D @ Vt).T
    return float(np.sqrt((np.square(a @ rot.T - b).sum(axis=1)).mean()))


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def ubq_ca():
    """the 76 CA atoms of 1ubq, read from the fixed columns of its ATOM records (no timed_hip involved)"""
    xyz = []
    with gzip.open(UBQ, "rt") as f:
        for line in f:
            if line.startswith("ATOM  ") and line[12:16].strip() == "CA" and line[16] in " A":
                xyz.append([float(line[30:38]), float(line[38:46]), float(line[46:54])])
            elif line.startswith("ENDMDL"):
                break
    return np.array(xyz, dtype=np.float64)


def rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


CASE_SEED = 5


def ubq_cases(seed=CASE_SEED):
    """{name: (ref, mob)}: the five cases of the tests, each a model of the 76 CA atoms of 1ubq in another frame"""
    ca = ubq_ca()
    rng = np.random.default_rng(seed)

    def placed(xyz):
        return xyz @ rotation(rng).T + rng.uniform(-20, 20, 3)
    cases = {"rigid": (ca, placed(ca)), "noise": (ca, placed(ca + rng.normal(0, 0.5, ca.shape)))}
    hinge = ca + rng.normal(0, 0.3, ca.shape)
    pivot = hinge[69].copy()
    hinge[69:] = (hinge[69:] - pivot) @ rotation(rng).T + pivot           # residues 70 onward re-oriented about residue 70
    cases["hinge"] = (ca, placed(hinge))
    cases["mirror"] = (ca, placed(ca * np.array([1.0, 1.0, -1.0])))
    broken = placed(ca + rng.normal(0, 0.5, ca.shape))
    broken[3, 1], broken[40, 0] = np.nan, np.inf
    ref = ca.copy()
    ref[11, 2], ref[40, 2] = -np.inf, np.nan
    cases["invalid"] = (ref, broken)
    return cases


def inputs_sha256(cases):
    h = hashlib.sha256()
    for name in CASES:
        for arr in cases[name]:
            h.update(np.ascontiguousarray(arr, dtype="<f8").tobytes())
    return h.hexdigest()


def golden_arrays(cases=None):
    """what tests/golden/superpose_golden.npz holds: the float64 restatement's outputs for every case, and the sha256 of the inputs"""
    cases = cases or ubq_cases()
    out = {"sha256": np.array(inputs_sha256(cases)), "cases": np.array(CASES)}
    for name in CASES:
        res = restate(*cases[name], cycles=CASE_CYCLES[name])
        for key in ("dist", "kept", "rmsd", "counts", "transform"):
            out[f"{name}_{key}"] = res[key]
    return out


SIZES = (0, 1, 2, 3, 4, 63, 64, 65, 76, 255, 256, 257, 1025)
RAGGED_SEED = 0


def synthetic_pair(n, rng, outliers=True):
    """a random-walk chain of n positions (3.8 Angstrom steps) against a rotated, translated copy with sigma = 1 Angstrom noise and,
    from 8 positions on, a few planted outliers 6 to 12 Angstrom off"""
    steps = rng.normal(size=(n, 3))
    steps *= 3.8 / np.maximum(np.linalg.norm(steps, axis=1, keepdims=True), 1e-9)
    ref = np.cumsum(steps, axis=0)
    mob = ref + rng.normal(0, 1.0, (n, 3))
    if outliers and n >= 8:
        where = rng.choice(n, size=max(1, n // 40), replace=False)
        kick = rng.normal(size=(len(where), 3))
        mob[where] += kick / np.linalg.norm(kick, axis=1, keepdims=True) * rng.uniform(6, 12, (len(where), 1))
    return ref, mob @ rotation(rng).T + rng.uniform(-30, 30, 3)


def ragged_batch(seed=RAGGED_SEED, copies=3):
    """about 40 pairs: every size of SIZES ``copies`` times with its own noise, in shuffled order -> [(ref, mob)]"""
    rng = np.random.default_rng(seed)
    pairs = [synthetic_pair(n, rng) for n in SIZES for _ in range(copies)]
    return [pairs[k] for k in rng.permutation(len(pairs))]


def flatten(pairs):
    """(ref [total, 3], mob [total, 3], offsets int64 [P + 1]) of a list of (ref, mob)"""
    offsets = np.concatenate([[0], np.cumsum([len(r) for r, _ in pairs])]).astype(np.int64)
    ref = np.concatenate([np.asarray(r, np.float64).reshape(-1, 3) for r, _ in pairs]) if pairs else np.zeros((0, 3))
    mob = np.concatenate([np.asarray(m, np.float64).reshape(-1, 3) for _, m in pairs]) if pairs else np.zeros((0, 3))
    return ref, mob, offsets


def degenerate_pairs(seed=2):
    """collinear chains and pairs of 1 and 2 positions: the RMSD is unique, the rotation is not"""
    rng = np.random.default_rng(seed)
    out = []
    for n in (1, 2, 2, 5, 40):
        t = np.sort(rng.uniform(-10, 10, n))[:, None]
        ref = t * np.array([[1.0, 2.0, -0.5]]) + np.array([3.0, -1.0, 7.0])
        mob = (t + rng.normal(0, 0.2, (n, 1))) * np.array([[-2.0, 0.3, 1.0]]) / np.linalg.norm([-2.0, 0.3, 1.0]) * np.linalg.norm([1.0, 2.0, -0.5])
        out.append((ref, mob + rng.uniform(-5, 5, 3)))
    return out


def pdb_text(xyz, names=None, chain="A", first=1):
    """ATOM records of a CA-only model (non-finite coordinates cannot be written: the caller leaves them out)"""
    lines = []
    for k, (x, y, z) in enumerate(np.asarray(xyz, np.float64)):
        res = names[k] if names else "GLY"
        lines.append(f"ATOM  {k + 1:5d}  CA  {res:>3s} {chain}{first + k:4d}    {x:8.3f}{y:8.3f}{z:8.3f}  1.00  0.00           C")
    return "\n".join(lines) + "\nEND\n"
