"""NumPy restatement of th_tag_rotamers (include/timed_hip.h): chi angles and rotamer classes of residues given as
``(residue name, [(atom name, xyz), ...])``.  Plain float64 (or np.longdouble for the chi-angle yardstick), one dict lookup per
path atom — independent of the kernel's method (no packed names, no flat arrays, no shared table: the paths are written out
again here).  Also the seeded synthetic residues and the exact-angle residues that tests/test_gpu_rotamers.py runs on the GPU."""
import hashlib
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
UBQ = os.path.join(HERE, "golden", "1ubq.pdb1.gz")
GOLDEN = os.path.join(HERE, "golden", "rotamer_tags_golden.npz")

# the 20 residues in the codec's order (by one-letter code) and the tail of each one's path behind N, CA, CB
TAILS = {"ALA": (), "CYS": ("SG",), "ASP": ("CG", "OD1"), "GLU": ("CG", "CD", "OE1"), "PHE": ("CG", "CD1"), "GLY": (),
         "HIS": ("CG", "ND1"), "ILE": ("CG1", "CD1"), "LYS": ("CG", "CD", "CE", "NZ"), "LEU": ("CG", "CD1"), "MET": ("CG", "SD", "CE"),
         "ASN": ("CG", "OD1"), "PRO": ("CG", "CD"), "GLN": ("CG", "CD", "OE1"), "ARG": ("CG", "CD", "NE", "CZ"), "SER": ("OG",),
         "THR": ("OG1",), "VAL": ("CG1",), "TRP": ("CG", "CD1"), "TYR": ("CG", "CD1")}
RESIDUES = list(TAILS)
CLASS_BASE = {}
_n = 0
for _res, _tail in TAILS.items():
    CLASS_BASE[_res] = _n
    _n += 3 ** len(_tail)
N_CLASSES = _n
EDGES = (0.0, 120.0, -120.0, 180.0, -180.0)


def path_of(res):
    return ("N", "CA", "CB") + TAILS[res] if TAILS.get(res) else ()


def dihedral(a, b, c, d, dtype=np.float64):
    """IUPAC dihedral of four points in degrees, (-180, 180]"""
    a, b, c, d = (np.asarray(v, dtype=dtype) for v in (a, b, c, d))
    b1, b2, b3 = b - a, c - b, d - c
    n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
    dot = lambda u, v: (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]          # noqa: E731
    with np.errstate(invalid="ignore", over="ignore"):
        return np.degrees(np.arctan2(np.sqrt(dot(b2, b2)) * dot(b1, n2), dot(n1, n2)))


def bin_of(chi):
    if 0 <= chi < 120:
        return 1
    if -120 <= chi < 0:
        return 3
    return 2


def restate(residues, ala_gly_class=True, dtype=np.float64):
    """-> (int16 [n] classes, dtype [n, 4] chi angles): the rule of th_tag_rotamers, residue by residue"""
    cls = np.full(len(residues), -1, np.int16)
    chi = np.full((len(residues), 4), np.nan, dtype=dtype)
    for r, (res, atoms) in enumerate(residues):
        if res not in TAILS:
            continue
        if not TAILS[res]:
            cls[r] = CLASS_BASE[res] if ala_gly_class else -1
            continue
        first = {}
        for name, pos in atoms:
            first.setdefault(name, pos)                                    # the first atom with a name wins
        path = path_of(res)
        if any(name not in first for name in path):
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            angles = [dihedral(*(first[name] for name in path[k:k + 4]), dtype=dtype) for k in range(len(path) - 3)]
        if not all(np.isfinite(x) for x in angles):
            continue
        index = 0
        for x in angles:
            index = index * 3 + (bin_of(x) - 1)                            # the first angle varies slowest
        cls[r] = CLASS_BASE[res] + index
        chi[r, :len(angles)] = angles
    return cls, chi


def edge_distance(chi):
    """smallest distance in degrees of any angle to a bin edge (0, +-120) or to the +-180 seam"""
    x = chi[np.isfinite(chi)].astype(np.float64)
    return min(float(np.abs(x - e).min()) for e in EDGES) if x.size else np.inf


def residues_of_model(model):
    """1ubq (or any pdbio.Model) as restate takes it: non-hetero residues, chains in file order"""
    chains = {}
    for r in model.residues:
        if not r.hetero:
            chains.setdefault(r.chain, []).append((r.name, list(r.atoms.items())))
    return [res for members in chains.values() for res in members]


def coords_sha256(residues):
    h = hashlib.sha256()
    for res, atoms in residues:
        h.update(res.encode())
        for name, pos in atoms:
            h.update(name.encode())
            h.update(np.asarray(pos, dtype="<f8").tobytes())
    return h.hexdigest()


def flatten(residues):
    """the arrays th_tag_rotamers takes, built without timed_hip: xyz, packed names, offsets, types"""
    xyz = np.array([pos for _, atoms in residues for _, pos in atoms], dtype=np.float64).reshape(-1, 3)
    names = np.array([int.from_bytes(name.encode("ascii")[:4].ljust(4, b"\0"), "little") for _, atoms in residues for name, _ in atoms],
                     dtype=np.uint32)
    offsets = np.concatenate([[0], np.cumsum([len(atoms) for _, atoms in residues])]).astype(np.int64)
    types = np.array([RESIDUES.index(res) if res in TAILS else -1 for res, _ in residues], dtype=np.int8)
    return xyz, names, offsets, types


SYNTH_SEED, SYNTH_COUNT = 11, 400


def synthetic_residues(seed=SYNTH_SEED, count=SYNTH_COUNT):
    """``count`` residues, every one of the 20 types at least ``count // 20`` times: random three-decimal coordinates for the path
    atoms and the backbone, hydrogens and OXT mixed in, file order shuffled, and for every third residue a DUPLICATE of one path
    name placed after the original (the first must win; the duplicate's coordinates would give another angle)."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        res = RESIDUES[k % 20]
        names = list(path_of(res) or ("N", "CA")) + ["C", "O"]
        atoms = [(name, np.round(rng.uniform(-4.0, 4.0, 3), 3)) for name in names]
        extra = [("H", rng.uniform(-4, 4, 3)), ("HA", rng.uniform(-4, 4, 3)), ("1HB", rng.uniform(-4, 4, 3)), ("OXT", rng.uniform(-4, 4, 3))]
        atoms += [(name, np.round(pos, 3)) for name, pos in extra[:int(rng.integers(0, 5))]]
        order = rng.permutation(len(atoms))
        atoms = [atoms[i] for i in order]
        if k % 3 == 0 and path_of(res):
            dup = path_of(res)[int(rng.integers(0, len(path_of(res))))]
            at = int(rng.integers([n for n, _ in atoms].index(dup) + 1, len(atoms) + 1))
            atoms.insert(at, (dup, np.round(rng.uniform(-4.0, 4.0, 3), 3)))
        out.append((res, atoms))
    return out


def serine_at(theta_deg):
    """a SER whose chi1 is theta (up to rounding): CA at the origin, CB on the x axis, N and OG one unit off the axis"""
    t = np.radians(np.float64(theta_deg))
    return ("SER", [("N", np.array([-0.5, 1.0, 0.0])), ("CA", np.zeros(3)), ("CB", np.array([1.5, 0.0, 0.0])),
                    ("OG", np.array([2.0, np.cos(t), np.sin(t)]))])
