"""The rule of th_seqset (include/timed_hip.h) restated in NumPy, written from the rule and NOT from the kernel: a broadcast compare for
M(i, j), plain Python loops for nearest, first_equal and the greedy clustering.  It makes tests/golden/seqset_golden.npz
(tests/golden/make_seqset_golden.py) and is what the GPU tests compare bytes with.  No GPU, no ctypes."""
import os

import numpy as np

from timed_hip.analysis import BLOSUM62, RESIDUES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "seqset_golden.npz")
UBQ = os.path.join(ROOT, "tests", "golden", "1ubq.pdb1.gz")
PHRASE = "THIS PROJECT'S OWN RULE, NOT THEIR CODE"
CASES = ("ubq_drift", "ubq_drift_07", "two_tiles", "long", "single", "empty", "all_same")
TABLES = ("seq", "profile", "set", "matrix")


def min_matches(per_mille, length):
    """ceil(p L / 1000) in integers"""
    return -((-int(per_mille) * int(length)) // 1000)


def pair_matches(codes):
    """[N, N] int32: M(i, j), by a broadcast compare, a block of rows at a time"""
    n = len(codes)
    out = np.zeros((n, n), np.int32)
    for lo in range(0, n, 32):
        out[lo:lo + 32] = (codes[lo:lo + 32, None, :] == codes[None, :, :]).sum(axis=2)
    return out


def restate(codes, native=None, threshold=None, substitution=BLOSUM62):
    """one set: dict of seq int32 [N, 8], profile int32 [L, 21], set int64 [4], matrix int32 [N, N]"""
    codes = np.asarray(codes, np.uint8)
    n, length = codes.shape
    assert length >= 1 and (codes <= 20).all()
    M = pair_matches(codes)
    seq = np.zeros((n, 8), np.int32)
    if native is not None:
        native = np.asarray(native, np.uint8)
        assert native.shape == (length,) and (native <= 20).all()
        for i in range(n):
            both = (codes[i] < 20) & (native < 20)
            scores = substitution[native[both].astype(int), codes[i][both].astype(int)].astype(np.int64)
            seq[i, 0] = int((codes[i] == native).sum())
            seq[i, 1] = int((scores > 0).sum())
            seq[i, 2] = int(scores.sum())
    representatives = []
    for i in range(n):
        others = [j for j in range(n) if j != i]
        seq[i, 3] = sum(int(M[i, j]) for j in others)
        seq[i, 4] = max((int(M[i, j]) for j in others), default=-1)
        seq[i, 5] = next((j for j in others if M[i, j] == seq[i, 4]), -1)
        seq[i, 6] = next(j for j in range(n) if M[i, j] == length)
        if threshold is None:
            seq[i, 7] = -1
        else:
            joined = next((r for r in representatives if M[i, r] >= threshold), None)
            if joined is None:
                representatives.append(i)
            seq[i, 7] = i if joined is None else joined
    profile = np.zeros((length, 21), np.int32)
    for c in range(21):
        profile[:, c] = (codes == c).sum(axis=0)
    totals = np.array([sum(int(M[i, j]) for i in range(n) for j in range(i + 1, n)), int((seq[:, 6] == np.arange(n)).sum()),
                       -1 if threshold is None else len(representatives), int(seq[:, 0].astype(np.int64).sum())], np.int64)
    return dict(seq=seq, profile=profile, set=totals, matrix=M)


def ubq_sequence():
    """the 76 codes of tests/golden/1ubq.pdb1.gz, read from the CA records of the fixed columns"""
    import gzip

    from design_utils.amino_acids import standard_amino_acids
    one = {three: letter for letter, three in standard_amino_acids.items()}
    with gzip.open(UBQ, "rt") as f:
        names = [line[17:20] for line in f if line[:6] == "ATOM  " and line[12:16] == " CA "]
    return np.array([RESIDUES.index(one[name]) for name in names], np.uint8)


def cases():
    """name -> (codes uint8 [N, L], native uint8 [L] or None, min_matches); the shapes are the smallest at which the kernel's 64 x 64
    tiles of sequences and 256-position chunks can go wrong (tests/test_gpu_seqset.py asserts that against the library's constants)"""
    out = {}
    native = ubq_sequence()
    rng = np.random.default_rng(2024)
    drift = np.tile(native, (70, 1))
    mutate = rng.random(drift.shape) < 0.15
    drift[mutate] = rng.integers(0, 20, int(mutate.sum())).astype(np.uint8)
    drift[5] = drift[2]
    drift[69] = drift[2]
    out["ubq_drift"] = (drift, native, min_matches(800, 76))
    out["ubq_drift_07"] = (drift, native, min_matches(700, 76))
    rng = np.random.default_rng(7)
    two = rng.integers(0, 3, (130, 9)).astype(np.uint8)                # three letters only: nearest ties abound
    two[3] = two[0]
    two[127] = two[0]
    out["two_tiles"] = (two, None, min_matches(900, 9))
    rng = np.random.default_rng(11)
    base = rng.integers(0, 20, 1030).astype(np.uint8)
    long = np.tile(base, (3, 1))
    change = rng.random(long.shape) < 0.3
    long[change] = rng.integers(0, 20, int(change.sum())).astype(np.uint8)
    long[rng.random(long.shape) < 0.05] = 20
    base = base.copy()
    base[rng.random(1030) < 0.05] = 20
    out["long"] = (long, base, min_matches(700, 1030))
    out["single"] = (np.array([[3, 20, 0, 19, 7]], np.uint8), np.array([3, 20, 1, 19, 20], np.uint8), min_matches(900, 5))
    out["empty"] = (np.zeros((0, 4), np.uint8), np.array([0, 5, 20, 19], np.uint8), min_matches(900, 4))
    out["all_same"] = (np.tile(np.array([4, 20, 0, 9], np.uint8), (66, 1)), np.array([4, 1, 0, 9], np.uint8), min_matches(900, 4))
    assert tuple(out) == CASES
    return out


def flatten(parts, natives=True):
    """(codes, seq_offsets, lengths, native or None, min_matches) of a list of cases for one call.  A case without a native gets code 20
    throughout when the call has one (its first three columns are then 0 all the same: nothing is known)"""
    offsets = np.zeros(len(parts) + 1, np.int64)
    np.cumsum([len(c) for c, _, _ in parts], out=offsets[1:])
    lengths = np.array([c.shape[1] for c, _, _ in parts], np.int32)
    codes = np.concatenate([c.reshape(-1) for c, _, _ in parts]) if parts else np.zeros(0, np.uint8)
    native = np.concatenate([n if n is not None else np.full(c.shape[1], 20, np.uint8) for c, n, _ in parts]) if natives else None
    return codes, offsets, lengths, native, np.array([t for _, _, t in parts], np.int32)


def golden_arrays():
    out = {"cases": np.array(CASES)}
    for name, (codes, native, threshold) in cases().items():
        got = restate(codes, native, threshold)
        out[f"{name}_codes"] = codes
        out[f"{name}_native"] = native if native is not None else np.zeros(0, np.uint8)
        out[f"{name}_min_matches"] = np.int32(threshold)
        for table in TABLES:
            out[f"{name}_{table}"] = got[table]
    return out
