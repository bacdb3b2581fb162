"""NumPy restatement of th_build_sidechains (include/timed_hip.h): side-chain heavy atoms placed from N, CA, C, the residue type and
the chi angles by internal coordinates; the deviation from native atoms of the same name; clash counts.  Plain float64 (or
np.longdouble for the yardstick), dicts keyed by atom NAME, residue after residue in Python loops — independent of the kernel's
method (no lanes, no levels, no packed names, no tiles) and of its table: the tree is written out again here and
tests/test_sidechains_host.py compares the two row for row.

    *** PARITY UNPINNED AGAINST SCWRL4 ***  The tree and its values are this project's own (standard stereochemistry after
    Engh & Huber 1991, branch offsets from the means of 1ubq); SCWRL4 is not available to pin them.

Also the 1ubq inputs, the table check (rebuild 1ubq from its native chi angles), ring closure and planarity, and the seeded
synthetic residues and structures that tests/test_gpu_sidechains.py runs on the GPU."""
import os

import numpy as np

import rotamer_restatement as rr

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "sidechain_golden.npz")
MAX_ATOMS = 10
CLASH_DISTANCE = 2.5

_CB = ("CB", ("C", "N", "CA"), -1, 1.530, 110.5, -122.5)


def _chain(*rows):
    """chi-path atoms behind CB: (name, bond length, bond angle) in path order; atom p[k + 3] hangs on p[k], p[k + 1], p[k + 2]"""
    path, out = ["N", "CA", "CB"], []
    for k, (name, length, angle) in enumerate(rows):
        out.append((name, tuple(path[k:k + 3]), k, length, angle, 0.0))
        path.append(name)
    return out


# residue -> rows (atom, (a, b, c), chi index or -1, |c d| in Angstrom, angle b-c-d in degrees, dihedral offset in degrees); the
# dihedral a-b-c-d is chi[k] + offset, or the offset alone when k is -1.  Build order; CB first.
TREE = {
    "ALA": [_CB],
    "CYS": [_CB] + _chain(("SG", 1.808, 114.4)),
    "ASP": [_CB] + _chain(("CG", 1.516, 112.6), ("OD1", 1.249, 118.4)) + [("OD2", ("CA", "CB", "CG"), 1, 1.249, 118.4, 180.0)],
    "GLU": [_CB] + _chain(("CG", 1.520, 114.1), ("CD", 1.516, 112.6), ("OE1", 1.249, 118.4)) + [("OE2", ("CB", "CG", "CD"), 2, 1.249, 118.4, 180.0)],
    "PHE": [_CB] + _chain(("CG", 1.502, 113.8), ("CD1", 1.384, 120.7)) + [
        ("CD2", ("CA", "CB", "CG"), 1, 1.384, 120.7, 180.0), ("CE1", ("CB", "CG", "CD1"), -1, 1.382, 120.7, 180.0),
        ("CE2", ("CB", "CG", "CD2"), -1, 1.382, 120.7, 180.0), ("CZ", ("CG", "CD1", "CE1"), -1, 1.382, 120.0, 0.0)],
    "GLY": [],
    "HIS": [_CB] + _chain(("CG", 1.497, 113.8), ("ND1", 1.378, 122.7)) + [
        ("CD2", ("CA", "CB", "CG"), 1, 1.354, 131.2, 180.0), ("CE1", ("CB", "CG", "ND1"), -1, 1.321, 109.0, 180.0),
        ("NE2", ("CB", "CG", "CD2"), -1, 1.374, 107.2, 180.0)],
    "ILE": [_CB] + _chain(("CG1", 1.530, 110.4), ("CD1", 1.513, 113.8)) + [("CG2", ("N", "CA", "CB"), 0, 1.521, 110.5, -124.0)],
    "LYS": [_CB] + _chain(("CG", 1.520, 114.1), ("CD", 1.520, 111.3), ("CE", 1.520, 111.3), ("NZ", 1.489, 111.9)),
    "LEU": [_CB] + _chain(("CG", 1.530, 116.3), ("CD1", 1.521, 110.7)) + [("CD2", ("CA", "CB", "CG"), 1, 1.521, 110.7, 122.0)],
    "MET": [_CB] + _chain(("CG", 1.520, 114.1), ("SD", 1.803, 112.7), ("CE", 1.791, 100.9)),
    "ASN": [_CB] + _chain(("CG", 1.516, 112.6), ("OD1", 1.231, 120.8)) + [("ND2", ("CA", "CB", "CG"), 1, 1.328, 116.4, 180.0)],
    "PRO": [_CB] + _chain(("CG", 1.492, 104.5), ("CD", 1.503, 106.1)),
    "GLN": [_CB] + _chain(("CG", 1.520, 114.1), ("CD", 1.516, 112.6), ("OE1", 1.231, 120.8)) + [("NE2", ("CB", "CG", "CD"), 2, 1.328, 116.4, 180.0)],
    "ARG": [_CB] + _chain(("CG", 1.520, 114.1), ("CD", 1.520, 111.3), ("NE", 1.460, 112.0), ("CZ", 1.329, 124.2)) + [
        ("NH1", ("CD", "NE", "CZ"), -1, 1.326, 120.0, 0.0), ("NH2", ("CD", "NE", "CZ"), -1, 1.326, 120.0, 180.0)],
    "SER": [_CB] + _chain(("OG", 1.417, 111.1)),
    "THR": [_CB] + _chain(("OG1", 1.433, 109.6)) + [("CG2", ("N", "CA", "CB"), 0, 1.521, 110.5, -120.5)],
    "VAL": [_CB] + _chain(("CG1", 1.521, 110.5)) + [("CG2", ("N", "CA", "CB"), 0, 1.521, 110.5, 123.0)],
    "TRP": [_CB] + _chain(("CG", 1.498, 113.6), ("CD1", 1.365, 126.9)) + [
        ("CD2", ("CA", "CB", "CG"), 1, 1.433, 126.8, 180.0), ("NE1", ("CB", "CG", "CD1"), -1, 1.374, 110.2, 180.0),
        ("CE2", ("CB", "CG", "CD2"), -1, 1.409, 107.2, 180.0), ("CE3", ("CB", "CG", "CD2"), -1, 1.398, 133.9, 0.0),
        ("CZ2", ("CG", "CD2", "CE2"), -1, 1.394, 122.4, 180.0), ("CZ3", ("CG", "CD2", "CE3"), -1, 1.382, 118.6, 180.0),
        ("CH2", ("CD2", "CE2", "CZ2"), -1, 1.368, 117.5, 0.0)],
    "TYR": [_CB] + _chain(("CG", 1.512, 113.9), ("CD1", 1.389, 120.8)) + [
        ("CD2", ("CA", "CB", "CG"), 1, 1.389, 120.8, 180.0), ("CE1", ("CB", "CG", "CD1"), -1, 1.382, 121.2, 180.0),
        ("CE2", ("CB", "CG", "CD2"), -1, 1.382, 121.2, 180.0), ("CZ", ("CG", "CD1", "CE1"), -1, 1.378, 119.6, 0.0),
        ("OH", ("CD1", "CE1", "CZ"), -1, 1.376, 119.9, 180.0)],
}
assert list(TREE) == rr.RESIDUES

# bonds the tree never uses: (atom, atom, stated length).  They close the rings, so they test the rows that lead to them.
CLOSURE = {"PHE": [("CE2", "CZ", 1.382)], "TYR": [("CE2", "CZ", 1.378)], "HIS": [("CE1", "NE2", 1.321)],
           "TRP": [("NE1", "CE2", 1.370), ("CZ3", "CH2", 1.400)]}
RINGS = {"PHE": ("CB", "CG", "CD1", "CD2", "CE1", "CE2", "CZ"), "TYR": ("CB", "CG", "CD1", "CD2", "CE1", "CE2", "CZ", "OH"),
         "HIS": ("CB", "CG", "ND1", "CD2", "CE1", "NE2"), "TRP": ("CB", "CG", "CD1", "CD2", "NE1", "CE2", "CE3", "CZ2", "CZ3", "CH2")}

CENTRES = {1: 60.0, 2: 180.0, 3: -60.0}


def n_chi_needed(res):
    return 1 + max((k for _, _, k, _, _, _ in TREE[res]), default=-1)


def dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def cross(u, v):
    return np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]], dtype=u.dtype)


def place(a, b, c, length, theta_deg, phi_deg, dtype=np.float64):
    """the atom d bonded to c with |cd| = length, angle b-c-d = theta and IUPAC dihedral a-b-c-d = phi (rr.dihedral's sign)"""
    a, b, c = (np.asarray(v, dtype=dtype) for v in (a, b, c))
    rad = np.arctan(dtype(1)) * 4 / dtype(180)                        # pi / 180 in the precision asked for
    theta, phi = dtype(theta_deg) * rad, dtype(phi_deg) * rad
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        bc = c - b
        bc = bc / np.sqrt(dot(bc, bc))
        n = cross(b - a, bc)
        n = n / np.sqrt(dot(n, n))
        m = cross(n, bc)
        x, y, z = -(length * np.cos(theta)), (length * np.sin(theta)) * np.cos(phi), (length * np.sin(theta)) * np.sin(phi)
        return c + ((x * bc + y * m) + z * n)


def build_residue(res, backbone, chi, dtype=np.float64):
    """{atom name: xyz} in build order, or None when the residue is unbuilt: not one of the 20, GLY, a backbone coordinate or a
    needed chi angle that is not finite, or any placed atom that is not finite (N, CA and C on a line)"""
    rows = TREE.get(res)
    if not rows:
        return None
    backbone = np.asarray(backbone, dtype=dtype)
    if not np.isfinite(backbone[:3].astype(np.float64)).all():
        return None
    atoms = {"N": backbone[0], "CA": backbone[1], "C": backbone[2]}
    built = {}
    for name, (a, b, c), k, length, angle, off in rows:
        phi = (dtype(chi[k]) if k >= 0 else dtype(0)) + dtype(off)
        atoms[name] = built[name] = place(atoms[a], atoms[b], atoms[c], dtype(length), angle, phi, dtype)
    if not all(np.isfinite(p.astype(np.float64)).all() for p in built.values()):
        return None
    return built


def restate_build(residues, dtype=np.float64):
    """``residues``: [(residue name, backbone [>= 3, 3], chi [4])] -> (dtype [n, 10, 3] NaN-padded, int32 [n] n_built)"""
    xyz = np.full((len(residues), MAX_ATOMS, 3), np.nan, dtype=dtype)
    n_built = np.zeros(len(residues), np.int32)
    for r, (res, backbone, chi) in enumerate(residues):
        built = build_residue(res, backbone, chi, dtype)
        if built:
            xyz[r, :len(built)] = list(built.values())
            n_built[r] = len(built)
    return xyz, n_built


def restate_match(residues, xyz, n_built, natives, dtype=np.float64):
    """``natives``: [(residue name, [(atom name, xyz), ...])] per residue -> (int32 [n] n_matched, dtype [n] sum_sq): every built
    atom against the FIRST native atom of its residue with its name, where the native residue is of the built type and the native
    atom is finite; squares summed in table order.  No symmetry correction."""
    n_matched = np.zeros(len(residues), np.int32)
    sum_sq = np.zeros(len(residues), dtype=dtype)
    for r, ((res, _, _), (native_res, atoms)) in enumerate(zip(residues, natives)):
        if not n_built[r] or native_res != res:
            continue
        first = {}
        for name, pos in atoms:
            first.setdefault(name, np.asarray(pos, dtype=dtype))
        for j, row in enumerate(TREE[res]):
            p = first.get(row[0])
            if p is None or not np.isfinite(p.astype(np.float64)).all():
                continue
            d = xyz[r, j].astype(dtype) - p
            sum_sq[r] = sum_sq[r] + dot(d, d)
            n_matched[r] += 1
    return n_matched, sum_sq


def restate_clashes(residues, xyz, chain_id, struct_offsets, clash_distance=CLASH_DISTANCE):
    """-> (int32 [n] clashes, int64 [S] pairs, float: the smallest | distance - clash_distance | met).  Atoms of a residue: its
    backbone rows (3 or 4) and its built side-chain atoms.  clashes[r] counts the pairs (side-chain atom of r, atom of another
    residue of the structure) closer than clash_distance (strict); between chain neighbours (consecutive residues with the same
    chain id) the other atom must be a side-chain atom too; SG-SG is never counted.  pairs[s]: the unordered pairs, once each."""
    clashes = np.zeros(len(residues), np.int32)
    pairs = np.zeros(len(struct_offsets) - 1, np.int64)
    margin = np.inf
    for s in range(len(struct_offsets) - 1):
        lo, hi = int(struct_offsets[s]), int(struct_offsets[s + 1])
        atoms = []                                                     # (residue, is side chain, name, xyz)
        for r in range(lo, hi):
            res, backbone, _ = residues[r]
            atoms += [(r, False, "bb", np.asarray(p, np.float64)) for p in np.asarray(backbone, np.float64)]
            if res in TREE:
                atoms += [(r, True, row[0], xyz[r, j].astype(np.float64)) for j, row in enumerate(TREE[res]) if np.isfinite(xyz[r, j]).all()]
        seen = set()
        for i, (ri, sc_i, name_i, pi) in enumerate(atoms):
            if not sc_i:
                continue
            for j, (rj, sc_j, name_j, pj) in enumerate(atoms):
                if rj == ri or (name_i == "SG" and name_j == "SG" and sc_j):
                    continue
                if abs(ri - rj) == 1 and chain_id[ri] == chain_id[rj] and not sc_j:
                    continue
                d = pj - pi
                with np.errstate(invalid="ignore", over="ignore"):
                    dist = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
                if np.isfinite(dist):
                    margin = min(margin, abs(float(dist) - clash_distance))
                if dist < clash_distance:
                    clashes[ri] += 1
                    seen.add((min(i, j), max(i, j)))
        pairs[s] = len(seen)
    return clashes, pairs, margin


# ---- the classes -------------------------------------------------------------------------------------------------------------------
def class_centres(cls):
    """class index -> (residue name, chi [4]: 60 / 180 / -60 for bins 1 / 2 / 3, NaN beyond the residue's angles)"""
    res = max((r for r in rr.RESIDUES if rr.CLASS_BASE[r] <= cls), key=lambda r: rr.CLASS_BASE[r])
    n, index = len(rr.TAILS[res]), cls - rr.CLASS_BASE[res]
    chi = [np.nan] * 4
    for k in range(n - 1, -1, -1):
        chi[k] = CENTRES[index % 3 + 1]
        index //= 3
    return res, np.array(chi)


# ---- 1ubq --------------------------------------------------------------------------------------------------------------------------
def ubq_inputs():
    """(residues as restate_build takes them with the native chi angles, natives as restate_match takes them, sha256)"""
    from timed_hip import pdbio
    natives = rr.residues_of_model(pdbio.read_pdb(rr.UBQ)[0])
    _, chi = rr.restate(natives)
    residues = []
    for (res, atoms), angles in zip(natives, chi):
        first = dict(reversed(atoms))
        residues.append((res, np.array([first[n] for n in ("N", "CA", "C", "O")], dtype=np.float64), angles))
    return residues, natives, rr.coords_sha256(natives)


def overall_rmsd(n_matched, sum_sq):
    return float(np.sqrt(np.asarray(sum_sq, np.float64).sum() / n_matched.sum()))


def closure_and_planarity(dtype=np.float64):
    """for every ring type on a fixed backbone and chi = (-65, 95): [(residue, atom, atom, stated, got)], {residue: worst distance
    of a ring atom from the least-squares plane of the ring atoms}"""
    backbone = np.array([[-0.525, 1.363, 0.0], [0.0, 0.0, 0.0], [1.526, 0.0, 0.0]])
    closures, planar = [], {}
    for res, ring in RINGS.items():
        built = build_residue(res, backbone, [-65.0, 95.0, np.nan, np.nan], dtype)
        for a, b, stated in CLOSURE[res]:
            d = (built[a] - built[b]).astype(np.float64)
            closures.append((res, a, b, stated, float(np.sqrt(d @ d))))
        pts = np.array([built[n] for n in ring], dtype=np.float64)
        pts = pts - pts.mean(0)
        normal = np.linalg.svd(pts)[2][-1]
        planar[res] = float(np.abs(pts @ normal).max())
    return closures, planar


# ---- synthetic inputs --------------------------------------------------------------------------------------------------------------
def random_backbone(rng, centre=(0.0, 0.0, 0.0)):
    """N, CA, C (and O) of one residue in a random orientation: bonds 1.458 / 1.525 / 1.231, N-CA-C between 90 and 150 degrees
    (redrawn otherwise), coordinates rounded to three decimals"""
    while True:
        q = rng.normal(size=(3, 3))
        e1 = q[0] / np.linalg.norm(q[0])
        e2 = q[1] - (q[1] @ e1) * e1
        e2 /= np.linalg.norm(e2)
        angle = np.radians(rng.uniform(100.0, 125.0))
        ca = np.asarray(centre, np.float64)
        n = ca + 1.458 * e1
        c = ca + 1.525 * (np.cos(angle) * e1 + np.sin(angle) * e2)
        o = c + 1.231 * np.cross(e1, e2)
        bb = np.round(np.array([n, ca, c, o]), 3)
        u, v = bb[0] - bb[1], bb[2] - bb[1]
        got = np.degrees(np.arccos(u @ v / np.linalg.norm(u) / np.linalg.norm(v)))
        if 90.0 <= got <= 150.0:
            return bb


def random_chi(rng):
    """four angles in (-180, 180), none within 1e-6 of +-180"""
    while True:
        chi = rng.uniform(-180.0, 180.0, 4)
        if (np.abs(np.abs(chi) - 180.0) > 1e-6).all():
            return chi


SYNTH_SEED, SYNTH_COUNT = 23, 200


def synthetic_residues(seed=SYNTH_SEED, count=SYNTH_COUNT):
    """``count`` residues, all 20 types in turn, on random backbones scattered over a 40 Angstrom box with random chi angles"""
    rng = np.random.default_rng(seed)
    return [(rr.RESIDUES[k % 20], random_backbone(rng, rng.uniform(-20.0, 20.0, 3)), random_chi(rng)) for k in range(count)]


def compact_structure(rng, n_res, spacing=4.2, types=None):
    """``n_res`` residues whose CA atoms sit on a jittered cubic lattice of ``spacing`` Angstrom — closer than side chains need, so
    they clash — with random types (no GLY) and chi angles; one chain"""
    side = int(np.ceil(n_res ** (1.0 / 3.0)))
    cells = [(x, y, z) for x in range(side) for y in range(side) for z in range(side)][:n_res]
    names = [r for r in rr.RESIDUES if r != "GLY"]
    out = []
    for k, cell in enumerate(cells):
        res = types[k] if types else names[int(rng.integers(0, len(names)))]
        out.append((res, random_backbone(rng, spacing * np.array(cell) + rng.uniform(-0.4, 0.4, 3)), random_chi(rng)))
    return out


def type_index(res):
    return rr.RESIDUES.index(res) if res in TREE else -1
