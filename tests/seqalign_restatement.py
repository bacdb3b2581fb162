"""The rule of th_seqalign (include/timed_hip.h) restated in plain Python / NumPy, written from the rule and NOT from the kernel: the
full H, E and F tables of the affine-gap alignment, the end cell, the trace, and the counts.  ``restate_plain`` is the rule cell by
cell; ``restate`` fills a row at a time (for the cases too large for a Python loop per cell) and is held to the plain one on the
fixture by tests/test_seqalign_host.py.  Both recompute the score FROM THE ALIGNMENT — the sum of S over the aligned pairs minus the
cost of every gap run on the path — and assert that it equals H at the end cell: a second, independent check of the trace.

    Which runs are on the path: in global mode all of them, the end runs included.  With free ends the path runs from the border cell
    where the trace stops to the end cell, and what lies outside it is free.  Every run strictly between the first and the last
    aligned pair is on it; beside those, a run of ONE side may precede the first pair or follow the last (a reference that starts
    PPPPPPPPPP and a model that starts WWWWW cannot both be skipped for nothing), and it is charged too.

It makes tests/golden/seqalign_golden.npz (tests/golden/make_seqalign_golden.py) and is what the GPU tests compare bytes with.  No GPU,
no ctypes.  *** PARITY UNPINNED AGAINST PYMOL ***"""
import os

import numpy as np

from timed_hip.analysis import BLOSUM62, RESIDUES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "seqalign_golden.npz")
UBQ = os.path.join(ROOT, "tests", "golden", "1ubq.pdb1.gz")
PHRASE = "PARITY UNPINNED AGAINST PYMOL"
NEG = -(1 << 30)
COUNT_COLUMNS = ("n_ref", "n_model", "score", "n_aligned", "n_identical", "n_positive", "n_gaps", "n_gap_residues")
TAG = "MHHHHHHSSG"
LINKER = "GSGSGSGSGS"


def default_matrix():
    """2 x BLOSUM62, -2 wherever either code is 20: written here from the issue's words, not imported from timed_hip.seqalign"""
    S = np.full((21, 21), -2, np.int32)
    S[:20, :20] = 2 * BLOSUM62.astype(np.int32)
    return S


def identity_matrix():
    """+1 on the diagonal of the 20 known codes, -1 elsewhere: the second table of the fixture (with gaps 3 / 1)"""
    S = np.full((21, 21), -1, np.int32)
    S[np.arange(20), np.arange(20)] = 1
    return S


def encode(text):
    return np.array([RESIDUES.index(c) if c in RESIDUES else 20 for c in str(text).upper()], np.uint8)


def cost(k, gap_open, gap_extend):
    return gap_open + (k - 1) * gap_extend if k > 0 else 0


def tables_plain(a, b, S, gap_open, gap_extend, free_ends):
    """H, E, F int64 [n + 1][m + 1], origin (0 diagonal, 1 F, 2 E) and the two extended bits, cell by cell"""
    n, m = len(a), len(b)
    H = [[0] * (m + 1) for _ in range(n + 1)]
    E = [[NEG] * (m + 1) for _ in range(n + 1)]
    F = [[NEG] * (m + 1) for _ in range(n + 1)]
    origin = [[0] * (m + 1) for _ in range(n + 1)]
    e_ext = [[False] * (m + 1) for _ in range(n + 1)]
    f_ext = [[False] * (m + 1) for _ in range(n + 1)]
    if not free_ends:
        for i in range(1, n + 1):
            H[i][0] = F[i][0] = -cost(i, gap_open, gap_extend)
        for j in range(1, m + 1):
            H[0][j] = E[0][j] = -cost(j, gap_open, gap_extend)
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            opened, extended = H[i][j - 1] - gap_open, E[i][j - 1] - gap_extend
            E[i][j] = max(opened, extended)
            e_ext[i][j] = extended > opened
            opened, extended = H[i - 1][j] - gap_open, F[i - 1][j] - gap_extend
            F[i][j] = max(opened, extended)
            f_ext[i][j] = extended > opened
            h, o = H[i - 1][j - 1] + int(S[a[i - 1]][b[j - 1]]), 0
            if F[i][j] > h:
                h, o = F[i][j], 1
            if E[i][j] > h:
                h, o = E[i][j], 2
            H[i][j], origin[i][j] = h, o
    return H, E, F, origin, e_ext, f_ext


def tables_rows(a, b, S, gap_open, gap_extend, free_ends):
    """the same tables a row at a time: E[i][j] = max over k < j of (max(diagonal, F)[i][k] - gap_open - (j - 1 - k) gap_extend), a
    running maximum (opening from an H that was itself an E is never above extending that E, as gap_open >= gap_extend); the bits
    are then read off the finished values by the rule's own comparisons"""
    n, m = len(a), len(b)
    H = np.zeros((n + 1, m + 1), np.int64)
    E = np.full((n + 1, m + 1), NEG, np.int64)
    F = np.full((n + 1, m + 1), NEG, np.int64)
    origin = np.zeros((n + 1, m + 1), np.int8)
    e_ext = np.zeros((n + 1, m + 1), bool)
    f_ext = np.zeros((n + 1, m + 1), bool)
    if not free_ends:
        H[1:, 0] = F[1:, 0] = -(gap_open + np.arange(n) * gap_extend)
        H[0, 1:] = E[0, 1:] = -(gap_open + np.arange(m) * gap_extend)
    if m == 0:
        return H, E, F, origin, e_ext, f_ext
    S = np.asarray(S, np.int64)
    b = np.asarray(b, np.int64)
    ramp = np.arange(m + 1, dtype=np.int64) * gap_extend
    for i in range(1, n + 1):
        opened, extended = H[i - 1, 1:] - gap_open, F[i - 1, 1:] - gap_extend
        F[i, 1:] = np.maximum(opened, extended)
        f_ext[i, 1:] = extended > opened
        part = H[i - 1, :-1] + S[int(a[i - 1])][b]                     # columns 1 .. m: the diagonal
        by_f = F[i, 1:] > part
        part = np.where(by_f, F[i, 1:], part)
        source = np.concatenate([[max(H[i, 0], E[i, 0] + gap_open - gap_extend)], part]) + ramp      # column 0 opens or extends
        E[i, 1:] = np.maximum.accumulate(source)[:-1] - gap_open - ramp[:-1]
        by_e = E[i, 1:] > part
        H[i, 1:] = np.where(by_e, E[i, 1:], part)
        origin[i, 1:] = np.where(by_e, 2, np.where(by_f, 1, 0))
        e_ext[i, 1:] = E[i, :-1] - gap_extend > H[i, :-1] - gap_open
    return H, E, F, origin, e_ext, f_ext


def finish(a, b, S, gap_open, gap_extend, free_ends, tables):
    """end cell, trace, counts and the score recomputed from the alignment"""
    H, E, F, origin, e_ext, f_ext = tables
    n, m = len(a), len(b)
    end = (n, m)
    if free_ends:
        for cell in [(n, j) for j in range(m - 1, -1, -1)] + [(i, m) for i in range(n - 1, -1, -1)]:
            if H[cell[0]][cell[1]] > H[end[0]][end[1]]:
                end = cell
    score = int(H[end[0]][end[1]])
    align = np.full(n, -1, np.int32)
    pairs = []
    i, j = end
    state = "H"
    while i > 0 and j > 0:
        if state == "H":
            o = int(origin[i][j])
            if o == 0:
                pairs.append((i, j))
                align[i - 1] = j - 1
                i, j = i - 1, j - 1
            else:
                state = "F" if o == 1 else "E"
        elif state == "F":
            state = "F" if f_ext[i][j] else "H"
            i -= 1
        else:
            state = "E" if e_ext[i][j] else "H"
            j -= 1
    stop = (i, j) if free_ends else (0, 0)
    pairs.reverse()
    # the score from the alignment: the pairs, and every run between the cell where the path starts and the end cell
    total = sum(int(S[a[p - 1]][b[q - 1]]) for p, q in pairs)
    n_gaps = n_gap_residues = 0
    walk = [stop] + pairs + [(end[0] + 1, end[1] + 1)]
    for k in range(len(walk) - 1):
        (p0, q0), (p1, q1) = walk[k], walk[k + 1]
        for run in (p1 - p0 - 1, q1 - q0 - 1):
            total -= cost(run, gap_open, gap_extend)
            if 0 < k < len(walk) - 2 and run > 0:                        # strictly between the first and the last aligned pair
                n_gaps += 1
                n_gap_residues += run
    assert total == score, (total, score, end, stop)
    counts = np.array([n, m, score, len(pairs), sum(int(a[p - 1] == b[q - 1]) for p, q in pairs),
                       sum(int(S[a[p - 1]][b[q - 1]] > 0) for p, q in pairs), n_gaps, n_gap_residues], np.int64)
    return dict(align=align, counts=counts, end=end, stop=stop)


def check_inputs(a, b, S, gap_open, gap_extend):
    a, b, S = np.asarray(a, np.uint8), np.asarray(b, np.uint8), np.asarray(S, np.int32)
    assert S.shape == (21, 21) and (np.abs(S) <= 127).all() and 0 <= gap_extend <= gap_open <= 32767
    assert a.ndim == b.ndim == 1 and (a <= 20).all() and (b <= 20).all() and max(len(a), len(b)) <= 4096
    return a, b, S


def restate_plain(a, b, S=None, gap_open=20, gap_extend=1, free_ends=1):
    a, b, S = check_inputs(a, b, default_matrix() if S is None else S, gap_open, gap_extend)
    return finish(a, b, S, gap_open, gap_extend, free_ends, tables_plain(a.tolist(), b.tolist(), S.tolist(), gap_open, gap_extend, free_ends))


def restate(a, b, S=None, gap_open=20, gap_extend=1, free_ends=1):
    a, b, S = check_inputs(a, b, default_matrix() if S is None else S, gap_open, gap_extend)
    return finish(a, b, S, gap_open, gap_extend, free_ends, tables_rows(a, b, S, gap_open, gap_extend, free_ends))


def restate_batch(ref_codes, ref_offsets, mob_codes, mob_offsets, S=None, gap_open=20, gap_extend=1, free_ends=1, fn=restate):
    """(align int32 [ref_total], counts int64 [pairs, 8]) of one flat call"""
    ref_codes, mob_codes = np.asarray(ref_codes, np.uint8), np.asarray(mob_codes, np.uint8)
    parts = [fn(ref_codes[int(ref_offsets[k]):int(ref_offsets[k + 1])], mob_codes[int(mob_offsets[k]):int(mob_offsets[k + 1])], S, gap_open,
                gap_extend, free_ends) for k in range(len(ref_offsets) - 1)]
    return (np.concatenate([p["align"] for p in parts] + [np.zeros(0, np.int32)]),
            np.array([p["counts"] for p in parts], np.int64).reshape(-1, 8))


def flatten(pairs):
    """(ref_codes, ref_offsets, mob_codes, mob_offsets) of a list of (a, b) code arrays"""
    ref_offsets, mob_offsets = np.zeros(len(pairs) + 1, np.int64), np.zeros(len(pairs) + 1, np.int64)
    np.cumsum([len(a) for a, _ in pairs], out=ref_offsets[1:])
    np.cumsum([len(b) for _, b in pairs], out=mob_offsets[1:])
    empty = [np.zeros(0, np.uint8)]
    return (np.concatenate([np.asarray(a, np.uint8) for a, _ in pairs] + empty), ref_offsets,
            np.concatenate([np.asarray(b, np.uint8) for _, b in pairs] + empty), mob_offsets)


def ubq_sequence():
    """the 76 letters of tests/golden/1ubq.pdb1.gz, read from the CA records of the fixed columns"""
    import gzip

    from design_utils.amino_acids import standard_amino_acids
    one = {three: letter for letter, three in standard_amino_acids.items()}
    with gzip.open(UBQ, "rt") as f:
        return "".join(one[line[17:20]] for line in f if line[:6] == "ATOM  " and line[12:16] == " CA ")


def mutate(codes, share, rng):
    out = np.array(codes, np.uint8)
    hit = rng.random(len(out)) < share
    out[hit] = (out[hit] + rng.integers(1, 20, int(hit.sum()))) % 20       # a substitution is never the same letter
    return out


def cases():
    """name -> (reference codes, model codes): the table of the rule, then mutated copies, an unrelated sequence, ties, the edges"""
    ubq = ubq_sequence()
    native = encode(ubq)
    deleted = np.concatenate([native[:22], native[28:]])                # residues 22 .. 27, counted from 0, are gone
    rng = np.random.default_rng(62)
    out = {"self": (native, native),
           "deletion": (native, deleted),
           "insertion": (native, encode(ubq[:33] + LINKER + ubq[33:])),        # after residue 32, counted from 0
           "tag": (native, encode(TAG + ubq)),
           "fragment": (native, native[20:60]),
           "mutated_30": (native, mutate(deleted, 0.3, rng)),
           "mutated_50": (native, mutate(deleted, 0.5, rng)),
           "mutated_70": (native, mutate(deleted, 0.7, rng)),
           "unrelated": (native, rng.integers(0, 20, 83).astype(np.uint8)),
           "poly_a": (encode("A" * 5), encode("A" * 9)),
           "poly_a_swapped": (encode("A" * 9), encode("A" * 5)),
           "two_letters": (rng.integers(0, 2, 23).astype(np.uint8), rng.integers(0, 2, 31).astype(np.uint8)),
           "two_letters_swapped": (rng.integers(0, 2, 37).astype(np.uint8), rng.integers(0, 2, 18).astype(np.uint8)),
           "reverse": (native, native[::-1].copy()),
           "overhangs": (encode("P" * 10 + ubq[:30]), encode("W" * 5 + ubq[:30])),      # a gap run before the first aligned pair, free ends or not
           "empty_both": (np.zeros(0, np.uint8), np.zeros(0, np.uint8)),
           "empty_reference": (np.zeros(0, np.uint8), native[:7]),
           "empty_model": (native[:7], np.zeros(0, np.uint8)),
           "one_one_same": (encode("W"), encode("W")),
           "one_one_other": (encode("W"), encode("P")),
           "one_many": (encode("K"), native[:12]),
           "many_one": (native[:12], encode("K")),
           "all_unknown": (np.full(9, 20, np.uint8), np.full(13, 20, np.uint8)),
           "unknown_in_known": (native[:30], np.concatenate([native[:10], np.full(4, 20, np.uint8), native[14:30]]))}
    return out


# (table, gap_open, gap_extend, free_ends) of every setting the fixture holds
SETTINGS = {"blosum_free": (default_matrix, 20, 1, 1), "blosum_global": (default_matrix, 20, 1, 0),
            "identity_free": (identity_matrix, 3, 1, 1), "identity_global": (identity_matrix, 3, 1, 0),
            "equal_costs_free": (identity_matrix, 2, 2, 1), "equal_costs_global": (identity_matrix, 2, 2, 0)}
# the prototype's figures: (score with free ends, global score, aligned residues)
TABLE = {"self": (762, 762, 76), "deletion": (681, 681, 70), "insertion": (733, 733, 76), "tag": (762, 733, 76), "fragment": (412, 338, 40)}


def golden_arrays(fn=restate_plain):
    out = {"cases": np.array(list(cases())), "settings": np.array(list(SETTINGS))}
    for name, (a, b) in cases().items():
        out[f"{name}_ref"], out[f"{name}_model"] = a, b
        for setting, (table, gap_open, gap_extend, free_ends) in SETTINGS.items():
            got = fn(a, b, table(), gap_open, gap_extend, free_ends)
            out[f"{name}_{setting}_align"], out[f"{name}_{setting}_counts"] = got["align"], got["counts"]
    return out


def restated_arrays(ref_codes, ref_offsets, mob_codes, mob_offsets, matrix=None, gap_open=20, gap_extend=1, free_ends=True, device=0, timing=None):
    """timed_hip.seqalign.seqalign_arrays with the GPU call replaced by the restatement"""
    from timed_hip import seqalign
    return seqalign.SeqalignTables(*restate_batch(ref_codes, np.asarray(ref_offsets), mob_codes, np.asarray(mob_offsets), matrix, int(gap_open),
                                                  int(gap_extend), int(bool(free_ends))))


def write_ubq_files(folder):
    """native.pdb; same/copy.pdb (renumbered from 101) and same/moved.pdb (shifted by 3 Angstrom): the native's sequence; and
    models/ with those two and deleted.pdb, which lacks residues 22 .. 27 counted from 0 — all through pdbio.write_pdb.
    -> the native's protein residues"""
    import copy

    from timed_hip import pdbio, structure
    protein = [r for r in structure.first_model(UBQ).residues if not r.hetero]

    def variant(residues, first=None, shift=0.0):
        out = copy.deepcopy(residues)
        for k, r in enumerate(out):
            r.atoms = {name: xyz + shift for name, xyz in r.atoms.items()}
            if first is not None:
                r.number = str(first + k)
        return pdbio.Model(1, out)
    for sub in ("same", "models"):
        (folder / sub).mkdir()
        pdbio.write_pdb(folder / sub / "copy.pdb", variant(protein, first=101))
        pdbio.write_pdb(folder / sub / "moved.pdb", variant(protein, shift=3.0))
    pdbio.write_pdb(folder / "native.pdb", pdbio.Model(1, protein))
    pdbio.write_pdb(folder / "models" / "deleted.pdb", variant(protein[:22] + protein[28:]))
    return protein
