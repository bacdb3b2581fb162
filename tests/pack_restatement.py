"""NumPy restatement of th_pack_sidechains (include/timed_hip.h): the rotamer search under the steric ladder and an optional prior.
An independent method: residues in Python loops, every candidate a dict {atom name: xyz} built by
``sidechain_restatement.build_residue`` from the class's centre angles, one candidate at a time against the atoms of the other
residues — no lanes, no tiles, no flat candidate array, no shared table.  Energies are recomputed FROM SCRATCH over residue pairs
(each pair once), not accumulated from the costs, so the two agree only if the bookkeeping is right.

    *** PARITY UNPINNED AGAINST SCWRL4 ***  The rule is this project's own; SCWRL4 is not available to pin it against.

``restate_pack`` returns the classes, every cost and energy, sweeps, moves, the energy after every move and the MARGIN: the
smallest | distance - level | over every pair of atoms it evaluated.  The kernel's outputs equal these as bytes when the margin
is above 1e-9 (float64 placement differences of about 1e-15 Angstrom cannot cross it): tests/test_pack_host.py checks that
condition for every input of tests/test_gpu_pack.py, all of which are made here (``gpu_cases``)."""
import os

import numpy as np

import rotamer_restatement as rr
import sidechain_restatement as sr

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "pack_golden.npz")
LADDER = (2.0, 2.5, 3.0, 3.5)
WEIGHT = 2000
MAX_SWEEPS = 10
MAX_CAND = 81
MAX_STRUCT = 4096
MARGIN_BOUND = 1e-9


def n_candidates(res):
    if res not in sr.TREE or not sr.TREE[res]:
        return 0
    return 3 ** len(rr.TAILS[res])


def candidates_of(res, backbone):
    """the candidates of one residue in class order: {atom name: xyz}, or None for one that is excluded; [] without any"""
    n = n_candidates(res)
    if n == 0 or not np.isfinite(np.asarray(backbone, np.float64)[:3]).all():
        return []
    out = []
    for k in range(n):
        name, chi = sr.class_centres(rr.CLASS_BASE[res] + k)
        assert name == res
        out.append(sr.build_residue(res, backbone, chi))
    return out


class _Penalty:
    """ladder levels between groups of atoms, with the margin of everything it has seen"""

    def __init__(self, ladder):
        self.ladder = np.asarray(ladder, np.float64)
        self.margin = np.inf

    def count(self, atoms, names, others, other_names):
        """atoms [a, 3] (names [a]) against others [m, 3] (other_names [m]): the levels under which each pair's distance lies,
        summed; SG-SG pairs are left out; a NaN is within nothing"""
        if not len(atoms) or not len(others):
            return 0
        d = others[None, :, :] - atoms[:, None, :]
        with np.errstate(invalid="ignore", over="ignore"):
            dist = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
        counted = ~((names[:, None] == "SG") & (other_names[None, :] == "SG"))
        seen = dist[counted & np.isfinite(dist)]
        if seen.size:
            self.margin = min(self.margin, float(np.abs(seen[:, None] - self.ladder[None, :]).min()))
        with np.errstate(invalid="ignore"):
            return int(((dist[..., None] < self.ladder) & counted[..., None]).sum())


def _arrays(cand):
    names = np.array(list(cand), dtype=object)
    return np.array([cand[n] for n in cand], np.float64).reshape(-1, 3), names


def restate_pack(residues, chain_id=None, ladder=LADDER, weight=WEIGHT, prior=None, max_sweeps=MAX_SWEEPS, limit=MAX_STRUCT):
    """ONE structure.  ``residues``: [(residue name or anything else, backbone [3 or 4, 3])]; ``chain_id`` [n] or None;
    ``prior`` int [n, 81] or None.  -> dict(cls, cost_initial, cost_final, energy_initial, energy_final, n_sweeps, n_moves,
    converged, status, margin, energies: the energy from scratch in the initial state and after every move)"""
    n = len(residues)
    out = dict(cls=np.full(n, -1, np.int16), cost_initial=np.zeros(n, np.int64), cost_final=np.zeros(n, np.int64), energy_initial=0,
               energy_final=0, n_sweeps=0, n_moves=0, converged=0, status=0, margin=np.inf, energies=[])
    if n > limit:
        out["status"] = 1
        return out
    chain_id = np.zeros(n, np.int64) if chain_id is None else np.asarray(chain_id)
    pen = _Penalty(ladder)
    weight = int(weight)
    cands = [[None if c is None else _arrays(c) for c in candidates_of(res, bb)] for res, bb in residues]
    valid = [[k for k, c in enumerate(cs) if c is not None] for cs in cands]
    cost_of_prior = lambda i, k: int(prior[i][k]) if prior is not None else 0          # noqa: E731
    bb_names = np.array(["bb"], dtype=object)

    def backbone_against(i):
        rows = [np.asarray(bb, np.float64) for j, (_, bb) in enumerate(residues)
                if j != i and not (abs(i - j) == 1 and chain_id[i] == chain_id[j])]
        return np.concatenate(rows) if rows else np.zeros((0, 3))
    bb_pen = []
    for i in range(n):
        others = backbone_against(i) if valid[i] else None
        bb_pen.append({k: pen.count(*cands[i][k], others, np.repeat(bb_names, len(others))) for k in valid[i]})

    state = [min(valid[i], key=lambda k: (cost_of_prior(i, k) + weight * bb_pen[i][k], k)) if valid[i] else -1 for i in range(n)]

    def side_chains_but(i):
        parts = [cands[j][state[j]] for j in range(n) if j != i and state[j] >= 0]
        if not parts:
            return np.zeros((0, 3)), np.zeros(0, dtype=object)
        return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])

    def cost(i, k, others):
        return cost_of_prior(i, k) + weight * (bb_pen[i][k] + pen.count(*cands[i][k], *others))

    pair_cache = {}

    def pair(i, j):
        key = (i, state[i], j, state[j])
        if key not in pair_cache:
            pair_cache[key] = pen.count(*cands[i][state[i]], *cands[j][state[j]])
        return pair_cache[key]

    def energy():
        chosen = [i for i in range(n) if state[i] >= 0]
        e = sum(cost_of_prior(i, state[i]) + weight * bb_pen[i][state[i]] for i in chosen)
        return e + weight * sum(pair(i, j) for a, i in enumerate(chosen) for j in chosen[a + 1:])

    def costs():
        return np.array([cost(i, state[i], side_chains_but(i)) if state[i] >= 0 else 0 for i in range(n)], np.int64)

    out["cost_initial"] = costs()
    out["energy_initial"] = energy()
    out["energies"].append(out["energy_initial"])
    movable = any(len(v) >= 2 for v in valid)
    out["converged"] = 0 if movable else 1
    if movable:
        for _ in range(int(max_sweeps)):
            moved = False
            for i in range(n):
                if len(valid[i]) < 2:
                    continue
                others = side_chains_but(i)
                table = {k: cost(i, k, others) for k in valid[i]}
                best = min(valid[i], key=lambda k: (table[k], k))
                if table[best] < table[state[i]]:
                    state[i] = best
                    moved = True
                    out["n_moves"] += 1
                    out["energies"].append(energy())
            out["n_sweeps"] += 1
            if not moved:
                out["converged"] = 1
                break
    out["cost_final"] = costs()
    out["energy_final"] = energy()
    out["cls"] = np.array([rr.CLASS_BASE[residues[i][0]] + state[i] if state[i] >= 0 else -1 for i in range(n)], np.int16)
    out["margin"] = pen.margin
    return out


def energy_from_scratch(residues, cls, chain_id=None, ladder=LADDER, weight=WEIGHT, prior=None):
    """the energy of the state ``cls`` without a search, a cache or a candidate list: every chosen side chain is built again from
    its class, met with every backbone that counts, and every pair of side chains is met once"""
    n = len(residues)
    chain_id = np.zeros(n, np.int64) if chain_id is None else np.asarray(chain_id)
    pen = _Penalty(ladder)
    total = 0
    built = []
    for i, (res, bb) in enumerate(residues):
        built.append(None)
        if cls[i] < 0:
            continue
        k = int(cls[i]) - rr.CLASS_BASE[res]
        atoms = _arrays(sr.build_residue(res, bb, sr.class_centres(int(cls[i]))[1]))
        built[i] = atoms
        total += int(prior[i][k]) if prior is not None else 0
        for j, (_, other) in enumerate(residues):
            if j != i and not (abs(i - j) == 1 and chain_id[i] == chain_id[j]):
                total += int(weight) * pen.count(*atoms, np.asarray(other, np.float64), np.repeat(np.array(["bb"], dtype=object), len(other)))
    for i in range(n):
        for j in range(i + 1, n):
            if built[i] is not None and built[j] is not None:
                total += int(weight) * pen.count(*built[i], *built[j])
    return total


def restate_batch(structures, **kw):
    """``structures``: [(residues, chain_id or None, prior or None)] -> the arrays of timed_hip.packer.PackedArrays as a dict, and
    the smallest margin"""
    parts = [restate_pack(res, chain, prior=prior, **kw) for res, chain, prior in structures]
    cat = lambda key, dtype: np.concatenate([np.asarray(p[key], dtype) for p in parts] + [np.zeros(0, dtype)])       # noqa: E731
    per = lambda key, dtype: np.array([p[key] for p in parts], dtype)                                                  # noqa: E731
    return dict(cls=cat("cls", np.int16), cost_initial=cat("cost_initial", np.int64), cost_final=cat("cost_final", np.int64),
                energy_initial=per("energy_initial", np.int64), energy_final=per("energy_final", np.int64), n_sweeps=per("n_sweeps", np.int32),
                n_moves=per("n_moves", np.int32), converged=per("converged", np.int32), status=per("status", np.int32)), \
        min([p["margin"] for p in parts] + [np.inf])


FIELDS = ("cls", "cost_initial", "cost_final", "energy_initial", "energy_final", "n_sweeps", "n_moves", "converged", "status")


def flat(structures):
    """[(residues, chain_id, prior)] as timed_hip.packer.pack_arrays takes them: backbone, types, offsets, chain ids, prior"""
    residues = [r for s in structures for r in s[0]]
    nb = len(residues[0][1]) if residues else 4
    backbone = np.array([r[1] for r in residues], np.float64).reshape(-1, nb, 3)
    types = np.array([sr.type_index(r[0]) for r in residues], np.int8)
    offsets = np.concatenate([[0], np.cumsum([len(s[0]) for s in structures])]).astype(np.int64)
    chain = np.concatenate([np.zeros(len(s[0]), np.int32) if s[1] is None else np.asarray(s[1], np.int32) for s in structures] + [np.zeros(0, np.int32)])
    priors = [s[2] for s in structures]
    prior = None
    if any(p is not None for p in priors):
        prior = np.concatenate([np.zeros((len(s[0]), MAX_CAND), np.int32) if s[2] is None else np.asarray(s[2], np.int32) for s in structures])
    return backbone, types, offsets, chain, prior


# ---- 1ubq and what the fixture holds ---------------------------------------------------------------------------------------------
def ubq_structure():
    """(residues [(name, backbone [4, 3])], native classes int16 [76], sha256)"""
    residues, natives, sha = sr.ubq_inputs()
    cls, _ = rr.restate(natives)
    return [(res, bb) for res, bb, _ in residues], cls, sha


def chi1_right(residues, cls, native_cls):
    """(residues of a type with a chi angle whose packed chi1 bin is the native's, residues with a chi angle and a native class)"""
    right = total = 0
    for (res, _), c, t in zip(residues, cls, native_cls):
        n_chi = len(rr.TAILS.get(res, ()))
        if n_chi == 0 or t < 0:
            continue
        total += 1
        if c >= 0:
            step = 3 ** (n_chi - 1)
            right += int((int(c) - rr.CLASS_BASE[res]) // step == (int(t) - rr.CLASS_BASE[res]) // step)
    return right, total


PRIOR_SEED, SEQUENCE_SEED = 41, 43


def synthetic_prior(residues, seed=PRIOR_SEED):
    """a seeded Dirichlet matrix [n, 338] through packer.prior_costs for the residues' own types"""
    from timed_hip import packer
    rng = np.random.default_rng(seed)
    matrix = rng.dirichlet(np.full(rr.N_CLASSES, 0.3), size=len(residues))
    return packer.prior_costs(matrix, [sr.type_index(res) for res, _ in residues])


def synthetic_sequence(residues, seed=SEQUENCE_SEED):
    """the backbones under seeded random residue types (all 20, GLY included)"""
    rng = np.random.default_rng(seed)
    return [(rr.RESIDUES[int(rng.integers(0, 20))], bb) for _, bb in residues]


def native_only_prior(residues, native_cls):
    """the prior under which the native class costs 0 and every other class the cap"""
    prior = np.full((len(residues), MAX_CAND), 10 ** 6, np.int32)
    for i, (res, _) in enumerate(residues):
        if native_cls[i] >= 0 and res in rr.CLASS_BASE:
            prior[i, int(native_cls[i]) - rr.CLASS_BASE[res]] = 0
    return prior


def fixture_cases():
    """name -> (residues, chain_id, prior, keywords of restate_pack): the four cases of tests/golden/pack_golden.npz"""
    residues, _, _ = ubq_structure()
    return {
        "native": (residues, None, None, {}),
        "prior": (residues, None, synthetic_prior(residues), {}),
        "predicted": (synthetic_sequence(residues), None, None, {}),
        "single_level": (residues, None, None, dict(ladder=(2.5,), weight=1)),
    }


# ---- the synthetic inputs of tests/test_gpu_pack.py --------------------------------------------------------------------------------
def compact(seed, n_res, types=None, spacing=4.2):
    rng = np.random.default_rng(seed)
    return [(res, bb) for res, bb, _ in sr.compact_structure(rng, n_res, spacing=spacing, types=types)]


RAGGED_SIZES = [1, 2, 0, 19, 37, 76]


def ragged_batch(seed=53):
    """structures of RAGGED_SIZES residues: ARG and LYS (81 candidates), an ALA / GLY-only structure, a residue of type -1 and one
    with a NaN backbone atom"""
    rng = np.random.default_rng(seed)
    out = []
    for s, n in enumerate(RAGGED_SIZES):
        part = [(res, bb) for res, bb, _ in sr.compact_structure(rng, n, spacing=5.5)]
        if n == 2:
            part = [("ALA", part[0][1]), ("GLY", part[1][1])]
        if n == 19:
            part[3] = ("ARG", part[3][1])
            part[4] = ("LYS", part[4][1])
            part[7] = ("HOH", part[7][1])
        if n == 37:
            bad = part[11][1].copy()
            bad[1, 2] = np.nan
            part[11] = ("LEU", bad)
            part[12] = ("ARG", part[12][1])
            part[20] = ("GLY", part[20][1])
        if n == 76:
            part[0] = ("LYS", part[0][1])
            part[75] = ("ARG", part[75][1])
        out.append((part, np.zeros(n, np.int32), None))
    return out


def many_small(seed=59, count=70):
    """``count`` structures of one or two residues"""
    rng = np.random.default_rng(seed)
    out = []
    for s in range(count):
        n = 1 + s % 2
        part = [(res, bb) for res, bb, _ in sr.compact_structure(rng, n, spacing=3.8)]
        out.append((part, np.zeros(n, np.int32), None))
    return out


def rule_cases(seed=61):
    """name -> structure (residues, chain_id, None): two LEU as chain neighbours and across a chain break; two CYS and two SER
    with their gamma atoms under the ladder"""
    rng = np.random.default_rng(seed)
    first = ("LEU", sr.random_backbone(rng))
    cb = sr.build_residue("LEU", first[1], [60.0, 60.0, np.nan, np.nan])["CB"]
    bb = sr.random_backbone(rng)
    second = ("LEU", bb + np.round(cb - bb[1] + np.array([0.6, 0.3, 0.2]), 3))
    out = {"neighbours": ([first, second], np.array([0, 0], np.int32), None), "chain_break": ([first, second], np.array([0, 1], np.int32), None)}
    base = sr.random_backbone(rng)
    for res in ("CYS", "SER"):
        out[res] = ([(res, base), (res, base + np.array([0.9, 0.8, -0.7]))], np.array([0, 1], np.int32), None)
    return out


def still_structure(seed=3):
    """ALA and GLY: nothing in it can move"""
    rng = np.random.default_rng(seed)
    return ([("ALA", sr.random_backbone(rng)), ("GLY", sr.random_backbone(rng, (9.0, 0.0, 0.0)))], None, None)


def limit_structures(seed=5):
    """a structure of one residue more than the per-structure limit, of residues without candidates so that it is cheap; one that
    is packed; one of exactly the limit"""
    rng = np.random.default_rng(seed)
    n = MAX_STRUCT + 1
    long = [("GLY", bb) for bb in np.repeat(sr.random_backbone(rng)[None], n, axis=0) + np.arange(n)[:, None, None] * 3.8]
    return [(long, None, None), (compact(67, 27), None, None), (long[:-1], None, None)]


def gpu_cases():
    """name -> ([(residues, chain_id, prior)], keywords): EVERY input that tests/test_gpu_pack.py packs, for the margin condition"""
    cases = {}
    for name, (residues, chain, prior, kw) in fixture_cases().items():
        cases["fixture_" + name] = ([(residues, chain, prior)], kw)
    ubq = fixture_cases()["native"][0]
    cases["cross_ubq"] = ([(ubq, None, None)], dict(ladder=(2.5,), weight=1))
    cases["cross_compact"] = ([(compact(67, 27), None, None)], dict(ladder=(2.5,), weight=1))
    cases["ragged"] = (ragged_batch(), {})
    cases["many_small"] = (many_small(), {})
    for name, structure in rule_cases().items():
        cases["rule_" + name] = ([structure], {})
    compact27 = compact(67, 27)
    cases["sweeps_0"] = ([(compact27, None, None)], dict(max_sweeps=0))
    cases["sweeps_1"] = ([(compact27, None, None)], dict(max_sweeps=1))
    cases["still"] = ([still_structure()], {})
    # more residues than the search kernel keeps in LDS (200): its atoms are streamed tile after tile, two tiles here, while the
    # small structure beside it, in the same launch, stays resident.  Mostly types of three candidates, to keep the restatement quick
    few = ["SER", "VAL", "THR", "CYS", "ALA", "SER", "VAL", "LEU", "THR", "ILE"]
    cases["streamed"] = ([(compact(71, 203, types=[few[k % 10] if k % 29 else "ARG" for k in range(203)]), None, None), (compact(73, 5), None, None)], {})
    cases["limit"] = (limit_structures(), {})
    return cases
