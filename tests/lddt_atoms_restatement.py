"""NumPy restatement of th_lddt_atoms (include/timed_hip.h): the all-atom local Distance Difference Test with the names of symmetric
side-chain atoms resolved per residue, one pair at a time, broadcast distances in float64 (or np.longdouble, to show that no decision
of a test sits where the precision matters).  Written from the header's rule, NOT from the kernel, and NOT by OpenStructure, which is
not available: the rule is this project's reading of the published definition (PARITY UNPINNED AGAINST OPENSTRUCTURE).

Also its own restatement of ``timed_hip.lddt_atoms.atom_lists`` for a pair of ``pdbio`` models (``lists_of_models``) and the cases of
tests/golden/lddt_atoms_golden.npz, built from tests/golden/1ubq.pdb1.gz or by hand."""
import hashlib
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
UBQ = os.path.join(HERE, "golden", "1ubq.pdb1.gz")
GOLDEN = os.path.join(HERE, "golden", "lddt_atoms_golden.npz")
PHRASE = "PARITY UNPINNED AGAINST OPENSTRUCTURE"
RADIUS = 15.0
THRESHOLDS = (0.5, 1.0, 2.0, 4.0)
EDGE = 1e-9                                # the float margin tests/test_gpu_lddt.py asks of the CA cases before it compares integers
BACKBONE = ("N", "CA", "C", "O")
# the table of the issue, restated: residue -> swappable name pairs
SYMMETRIC = {"ASP": (("OD1", "OD2"),), "GLU": (("OE1", "OE2"),), "PHE": (("CD1", "CD2"), ("CE1", "CE2")), "TYR": (("CD1", "CD2"), ("CE1", "CE2")),
             "ARG": (("NH1", "NH2"),), "LEU": (("CD1", "CD2"),), "VAL": (("CG1", "CG2"),)}
INPUTS = ("ref", "mob", "residue", "partner")
TABLES = ("atom", "swapped", "pair")


def distances(a, b):
    """d[i, j] = sqrt((dx*dx + dy*dy) + dz*dz) between a[i] and b[j], in the arrays' dtype"""
    dx = b[None, :, 0] - a[:, None, 0]
    dy = b[None, :, 1] - a[:, None, 1]
    dz = b[None, :, 2] - a[:, None, 2]
    return np.sqrt((dx * dx + dy * dy) + dz * dz)


def restate(ref, mob, residue, partner, radius=RADIUS, thresholds=THRESHOLDS, symmetry=True, dtype=np.float64):
    """The rule of th_lddt_atoms on one pair.  Returns a dict: ``atom`` [n, 5] int32 (n_i, c_i[0..3]), ``swapped`` [n] uint8, ``pair``
    [8] int64 (n_ref, n_missing, N, C[0..3], n_swapped_residues), ``keep`` / ``swap`` {residue: sum}, ``edge`` — the smallest of
    |d_ref - radius| over the ordered pairs of reference-valid atoms of different residues and of ||d_ref - d_mob| - t| over the
    included pairs with a finite model distance, under either naming of a symmetric residue, and the four thresholds (inf when there
    is none) — and ``margin``: the smallest |swap_R - keep_R| over the symmetric residues (inf when there is none)."""
    ref = np.asarray(ref, dtype=np.float64).reshape(-1, 3)
    mob = np.asarray(mob, dtype=np.float64).reshape(-1, 3).copy()
    residue, partner = np.asarray(residue, dtype=np.int64).reshape(-1), np.asarray(partner, dtype=np.int64).reshape(-1)
    n = len(ref)
    assert mob.shape == ref.shape and len(residue) == n and len(partner) == n and len(thresholds) == 4
    valid = np.isfinite(ref).all(axis=1)
    missing = valid & ~np.isfinite(mob).all(axis=1)
    mob[~np.isfinite(mob).all(axis=1)] = np.nan                          # a missing atom: all three NaN
    limits = [dtype(t) for t in thresholds]
    edge, margin = np.inf, np.inf
    keep, swap = {}, {}
    atom, swapped = np.zeros((n, 5), np.int32), np.zeros(n, np.uint8)
    with np.errstate(over="ignore", invalid="ignore"):
        d_ref = distances(ref.astype(dtype), ref.astype(dtype))
        candidates = valid[:, None] & valid[None, :] & (residue[:, None] != residue[None, :])
        included = candidates & (d_ref < dtype(radius))
        if candidates.any():
            edge = min(edge, float(np.abs(d_ref - dtype(radius))[candidates].min()))

        def preserved(d_mob, mask):
            """[4] counts of the masked pairs preserved at each threshold; the edge takes every finite difference of the mask"""
            nonlocal edge
            diff = np.abs(d_ref_part - d_mob)
            finite = mask & np.isfinite(diff)
            for t in limits:
                if finite.any():
                    edge = min(edge, float(np.abs(diff - t)[finite].min()))
            return [mask & (diff < t) for t in limits]
        used = mob.copy()
        if symmetry:
            free = partner < 0
            for r in np.unique(residue[partner >= 0]).tolist():
                a = np.flatnonzero((residue == r) & (partner >= 0))
                b = np.flatnonzero(free & (residue != r))
                mask, d_ref_part = included[np.ix_(a, b)], d_ref[np.ix_(a, b)]
                keep[r] = int(sum(m.sum() for m in preserved(distances(mob[a].astype(dtype), mob[b].astype(dtype)), mask)))
                swap[r] = int(sum(m.sum() for m in preserved(distances(mob[partner[a]].astype(dtype), mob[b].astype(dtype)), mask)))
                margin = min(margin, abs(swap[r] - keep[r]))
                if swap[r] > keep[r]:                                   # a tie keeps the names
                    used[a] = mob[partner[a]]
                    swapped[a] = 1
        d_ref_part = d_ref
        hits = preserved(distances(used.astype(dtype), used.astype(dtype)), included)
    atom[:, 0] = included.sum(axis=1)
    for k in range(4):
        atom[:, 1 + k] = hits[k].sum(axis=1)
    assert not atom[~valid].any()
    flipped = sum(1 for r in keep if swap[r] > keep[r])
    pair = np.concatenate([[int(valid.sum()), int(missing.sum())], atom.astype(np.int64).sum(axis=0), [flipped]]).astype(np.int64)
    return dict(atom=atom, swapped=swapped, pair=pair, keep=keep, swap=swap, edge=edge, margin=margin)


def restate_batch(ref, mob, residue, partner, offsets, radius=RADIUS, thresholds=THRESHOLDS, symmetry=True, dtype=np.float64):
    """the tables th_lddt_atoms returns for a flat batch: (atom [total, 5] int32, swapped [total] uint8, pair [P, 8] int64)"""
    ref, mob = np.asarray(ref, np.float64).reshape(-1, 3), np.asarray(mob, np.float64).reshape(-1, 3)
    offsets = np.asarray(offsets, np.int64).reshape(-1)
    parts = [restate(ref[lo:hi], mob[lo:hi], residue[lo:hi], partner[lo:hi], radius, thresholds, symmetry, dtype)
             for lo, hi in zip(offsets[:-1], offsets[1:])]
    atom = np.concatenate([p["atom"] for p in parts]) if parts else np.zeros((0, 5), np.int32)
    swapped = np.concatenate([p["swapped"] for p in parts]) if parts else np.zeros(0, np.uint8)
    pair = np.stack([p["pair"] for p in parts]) if parts else np.zeros((0, 8), np.int64)
    return atom, swapped, pair


def score(pair):
    """lddt = sum_k C[k] / (4 N) of one row of the pair table, NaN when N = 0"""
    return float(pair[3:7].sum()) / (4.0 * float(pair[2])) if pair[2] else float("nan")


def flatten(cases):
    """[case dict] -> (ref, mob, residue, partner, offsets) of one batch"""
    offsets = np.concatenate([[0], np.cumsum([len(c["ref"]) for c in cases])]).astype(np.int64)
    return (np.concatenate([c["ref"].reshape(-1, 3) for c in cases]), np.concatenate([c["mob"].reshape(-1, 3) for c in cases]),
            np.concatenate([c["residue"] for c in cases]).astype(np.int32), np.concatenate([c["partner"] for c in cases]).astype(np.int32), offsets)


# ---- the atoms of a pair of pdbio models, restated from the issue's rules ----------------------------------------------------------

def is_hydrogen(res, name):
    element = (res.elements.get(name) or "").strip().upper()
    if not element or not element[0].isalpha():
        element = name.lstrip("0123456789 ")[:1].upper()
    return element in ("H", "D")


def lists_of_models(reference, model):
    """(ref [n, 3], mob [n, 3], residue [n], partner [n], backbone [n] bool, n_mismatched_residues) of two pdbio models whose non-hetero
    residues are paired by position"""
    ours = [r for r in reference.residues if not r.hetero]
    theirs = [r for r in model.residues if not r.hetero]
    assert len(ours) == len(theirs)
    ref, mob, residue, partner, backbone = [], [], [], [], []
    mismatched = index = 0
    for a, b in zip(ours, theirs):
        names = [name for name in a.atoms if name != "OXT" and not is_hydrogen(a, name)]
        if a.name != b.name:
            mismatched += 1
            names = [name for name in names if name in BACKBONE]
        if not names:
            continue
        first = len(ref)
        for name in names:
            ref.append(a.atoms[name])
            mob.append(b.atoms[name] if name in b.atoms else [np.nan] * 3)
            residue.append(index)
            backbone.append(name in BACKBONE)
            other = -1
            if a.name == b.name:
                for x, y in SYMMETRIC.get(a.name, ()):
                    if name in (x, y) and x in names and y in names:
                        other = first + names.index(y if name == x else x)
            partner.append(other)
        index += 1
    return (np.array(ref, np.float64).reshape(-1, 3), np.array(mob, np.float64).reshape(-1, 3), np.array(residue, np.int32),
            np.array(partner, np.int32), np.array(backbone, bool), mismatched)


def ubq():
    from timed_hip import pdbio
    return pdbio.read_pdb(UBQ)[0]


def exchanged(mob, partner):
    """the model with every symmetric name pair exchanged: atom i carries the coordinates its partner had"""
    out = np.array(mob, np.float64, copy=True)
    has = partner >= 0
    out[has] = mob[partner[has]]
    return out


def synthetic_chain(sizes, partnered, seed, sigma=0.4, flipped=()):
    """A chain of residues of ``sizes`` atoms on a random walk (steps of about 1.5 Angstrom), the model its noisy copy; ``partnered``:
    (atom, atom) pairs inside one residue; the pairs whose index is in ``flipped`` have exchanged coordinates in the model."""
    rng = np.random.default_rng(seed)
    n = int(sum(sizes))
    ref = np.cumsum(rng.normal(0.0, 0.9, (n, 3)), axis=0)
    mob = ref + rng.normal(0.0, sigma, (n, 3))
    residue = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    partner = np.full(n, -1, np.int32)
    for k, (a, b) in enumerate(partnered):
        assert residue[a] == residue[b] and a != b
        partner[a], partner[b] = b, a
        if k in flipped:
            mob[[a, b]] = mob[[b, a]]
    return dict(ref=ref, mob=mob, residue=residue, partner=partner)


def hand_cases():
    """From exactly representable numbers (3-4-5 and 9-12-15 triangles, quarters): name -> (case, atom rows, swapped, pair row)"""
    none2, none4 = np.full(2, -1, np.int32), np.full(4, -1, np.int32)
    o = [0.0, 0.0, 0.0]
    out = {}
    # a structure of a single residue: nothing is included, the score is NaN
    one = np.array([o, [1.5, 0.0, 0.0], [0.0, 1.5, 0.0]])
    out["hand_single_residue"] = (dict(ref=one, mob=one + 0.25, residue=np.zeros(3, np.int32), partner=np.array([-1, 2, 1], np.int32)),
                                  [[0] * 5] * 3, [0, 0, 0], [3, 0, 0, 0, 0, 0, 0, 0])
    # two residues of two atoms on a line: d_ref 4, 6, 3, 5 against d_mob 4.25, 7.5, 3.25, 6.5: differences 0.25, 1.5, 0.25, 1.5
    line = lambda xs: np.array([[x, 0.0, 0.0] for x in xs])                # noqa: E731
    out["hand_two_residues"] = (dict(ref=line([0.0, 1.0, 4.0, 6.0]), mob=line([0.0, 1.0, 4.25, 7.5]), residue=np.array([0, 0, 1, 1], np.int32),
                                     partner=none4), [[2, 1, 1, 2, 2], [2, 1, 1, 2, 2], [2, 2, 2, 2, 2], [2, 0, 0, 2, 2]], [0] * 4,
                                [4, 0, 8, 4, 4, 8, 8, 0])
    # two atoms at exactly the radius: excluded
    far = np.array([o, [9.0, 12.0, 0.0]])
    out["hand_at_the_radius"] = (dict(ref=far, mob=far, residue=np.array([0, 1], np.int32), partner=none2), [[0] * 5] * 2, [0, 0],
                                 [2, 0, 0, 0, 0, 0, 0, 0])
    # a difference of exactly a threshold: d_ref 5, d_mob 5.5: not preserved at 0.5
    out["hand_at_a_threshold"] = (dict(ref=np.array([o, [3.0, 4.0, 0.0]]), mob=np.array([o, [0.0, 0.0, 5.5]]), residue=np.array([0, 1], np.int32),
                                       partner=none2), [[1, 0, 1, 1, 1]] * 2, [0, 0], [2, 0, 2, 0, 2, 2, 2, 0])
    # a symmetric residue whose two namings preserve the same: both partners 5 from the one other atom, in both structures
    tie = np.array([[3.0, 0.0, 0.0], [-3.0, 0.0, 0.0], [0.0, 4.0, 0.0]])
    out["hand_swap_tie"] = (dict(ref=tie, mob=tie, residue=np.array([0, 0, 1], np.int32), partner=np.array([1, 0, -1], np.int32)),
                            [[1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [2, 2, 2, 2, 2]], [0, 0, 0], [3, 0, 4, 4, 4, 4, 4, 0])
    return out


TIES = ("hand_single_residue", "hand_two_residues", "hand_at_the_radius", "hand_at_a_threshold", "hand_swap_tie")
MARGIN_TIES = ("missing_symmetric",)                          # swap_R == keep_R == 0 by construction; the float margin is still asked
TEN_RESIDUES = (0, 1, 2, 5, 10, 12, 24, 30, 47, 67)           # positions of 1ubq (M Q I K K I N Q K H: none symmetric) whose side chains
#                                                               beyond CB the model of case 4 lacks
TEN_SYMMETRIC = (3, 11, 17, 26, 32, 40, 44, 53, 62, 70)       # ... and ten with PHE 4, GLU 18, PHE 45, ARG 54 and LEU 71 among them: a
#                                                               symmetric residue without its partnered atoms is a tie at 0 = 0
FIVE_RESIDUES = (5, 14, 44, 58, 66)                           # positions renamed in the model of case 6


def build_cases():
    """name -> dict(ref, mob, residue, partner [, backbone, n_mismatched]): every case of the fixture, in its order"""
    import copy
    native = ubq()
    ref, _, residue, partner, backbone, mismatched = lists_of_models(native, native)
    assert mismatched == 0
    base = dict(ref=ref, residue=residue, partner=partner, backbone=backbone)
    cases = {"self": dict(base, mob=ref.copy()), "flipped": dict(base, mob=exchanged(ref, partner))}
    noisy = ref + np.random.default_rng(20130101).normal(0.0, 0.3, ref.shape)
    cases["noise"] = dict(base, mob=noisy)
    cases["noise_flipped"] = dict(base, mob=exchanged(noisy, partner))
    # case 4: the model lacks the side chains beyond CB of ten residues
    kept = BACKBONE + ("CB",)

    def without_side_chains(positions):
        short = copy.deepcopy(native)
        for k in positions:
            short.residues[k].atoms = {name: xyz for name, xyz in short.residues[k].atoms.items() if name in kept}
        return lists_of_models(native, short)
    lacking = without_side_chains(TEN_RESIDUES)
    cases["missing"] = dict(base, mob=lacking[1], partner=lacking[3])
    cases["missing_symmetric"] = dict(base, mob=without_side_chains(TEN_SYMMETRIC)[1])
    infinite = lacking[1].copy()
    gone = np.flatnonzero(np.isnan(infinite).any(axis=1))
    infinite[gone] = ref[gone]
    infinite[gone, np.arange(len(gone)) % 3] = np.where(np.arange(len(gone)) % 2, np.inf, -np.inf)       # one coordinate of each
    cases["missing_infinite"] = dict(base, mob=infinite, partner=lacking[3])
    # case 5: non-finite reference coordinates, a partnered atom among them
    broken = ref.copy()
    for n, i in enumerate((0, 7, 100, 257, 600, int(np.flatnonzero(partner >= 0)[5]))):
        broken[i, n % 3] = (np.nan, np.inf, -np.inf)[n % 3]
    cases["reference_invalid"] = dict(base, ref=broken, mob=noisy)
    # case 6: five residues renamed in the model: only their backbone enters
    renamed = copy.deepcopy(native)
    for k in FIVE_RESIDUES:
        renamed.residues[k].name = "ALA" if renamed.residues[k].name != "ALA" else "SER"
    got = lists_of_models(native, renamed)
    rng = np.random.default_rng(66)
    cases["renamed"] = dict(ref=got[0], mob=got[1] + rng.normal(0.0, 0.3, got[1].shape), residue=got[2], partner=got[3], backbone=got[4],
                            n_mismatched=np.array(got[5]))
    for name, (case, _, _, _) in hand_cases().items():
        cases[name] = case
    # case 8: tile edges (the kernels' tile is 256 atoms)
    cases["chain_257"] = synthetic_chain([3] * 85 + [2], [(255, 256), (0, 2), (30, 31), (126, 128)], seed=257, flipped=(0, 2))
    sizes_300 = [2] * 127 + [5] + [2] * 20 + [1]
    cases["chain_300"] = synthetic_chain(sizes_300, [(254, 258), (255, 257), (0, 1), (100, 101), (297, 298)], seed=300, flipped=(0, 1, 3))
    cases["chain_256"] = synthetic_chain([4] * 64, [(0, 3), (252, 255), (129, 130)], seed=256, flipped=(1,))
    cases["chain_1"] = synthetic_chain([1], [], seed=1)
    return cases


def inputs_sha256(cases):
    h = hashlib.sha256()
    for name, case in cases.items():
        h.update(name.encode())
        for key in INPUTS:
            h.update(np.ascontiguousarray(case[key]).tobytes())
    return h.hexdigest()


def golden_arrays(cases=None):
    """what tests/golden/lddt_atoms_golden.npz holds: every case's inputs, its resolved tables and its tables as named, and the
    sha256 of the inputs"""
    cases = cases or build_cases()
    out = {"sha256": np.array(inputs_sha256(cases)), "cases": np.array(list(cases))}
    for name, case in cases.items():
        out[f"{name}_ref"], out[f"{name}_mob"] = np.asarray(case["ref"], np.float64), np.asarray(case["mob"], np.float64)
        out[f"{name}_residue"], out[f"{name}_partner"] = np.asarray(case["residue"], np.int32), np.asarray(case["partner"], np.int32)
        for key in ("backbone", "n_mismatched"):
            if key in case:
                out[f"{name}_{key}"] = np.asarray(case[key])
        for tag, symmetry in (("", True), ("_named", False)):
            res = restate(*(case[key] for key in INPUTS), symmetry=symmetry)
            for table in TABLES:
                out[f"{name}{tag}_{table}"] = res[table]
    return out


def golden_cases(golden):
    """the fixture's cases as dicts of inputs, in its order"""
    return {str(name): {key: golden[f"{name}_{key}"] for key in INPUTS} for name in golden["cases"].tolist()}
