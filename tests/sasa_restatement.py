"""NumPy restatement of th_sasa (include/timed_hip.h): solvent-accessible surface by Shrake & Rupley (1973) on the atoms of one
structure at a time — expanded radii, the near pre-filter, sphere points, strict occlusion, counts, masks and totals.  Plain NumPy;
every float64 product, sum and difference is one NumPy operation, so each is rounded on its own, in the order the rule writes them.
Computed by this file, NOT by FreeSASA, NACCESS, DSSP or Biopython, none of which is available: the rule is this project's own
(PARITY UNPINNED AGAINST FREESASA / NACCESS / DSSP / BIOPYTHON).

The result is an AND over neighbours, so the order in which pairs are visited cannot change a bit: they are visited nearest first,
in chunks, and an atom whose points are all buried is not visited again.

Also the inputs of the tests: the heavy atoms of tests/golden/1ubq.pdb1.gz read from the fixed columns of its records (no timed_hip
involved), a rigidly moved copy of them (the dimer), a three-atom pseudo-ligand on the first three water sites, the analytic cases of
the rule's write-up, and the cuts of the length batch."""
import gzip
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
UBQ = os.path.join(HERE, "golden", "1ubq.pdb1.gz")
GOLDEN = os.path.join(HERE, "golden", "sasa_golden.npz")
PHRASE = "PARITY UNPINNED AGAINST FREESASA / NACCESS / DSSP / BIOPYTHON"
RADII = {"C": 1.70, "N": 1.55, "O": 1.52, "S": 1.80, "P": 1.80, "SE": 1.90}
OTHER_RADIUS = 1.80
MAX_ASA = {"ALA": 129.0, "ARG": 274.0, "ASN": 195.0, "ASP": 193.0, "CYS": 167.0, "GLN": 225.0, "GLU": 223.0, "GLY": 104.0, "HIS": 224.0,
           "ILE": 197.0, "LEU": 201.0, "LYS": 236.0, "MET": 224.0, "PHE": 240.0, "PRO": 159.0, "SER": 155.0, "THR": 172.0, "TRP": 285.0,
           "TYR": 263.0, "VAL": 174.0}
WATERS = ("HOH", "WAT", "DOD")
PROBE = 1.4
CASES = ("ubq", "ubq_960", "ubq_probe0", "ubq_dimer", "ubq_hetero", "lone", "pair_3", "pair_6", "inside", "tie", "tie_near")
# the exposed counts the rule's write-up states for the analytic cases
ANALYTIC = {"lone": [96], "pair_3": [72, 72], "pair_6": [96, 96], "inside": [0, 96], "tie": [3, 3], "tie_near": [2, 2]}
BATCH_LENGTHS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 602)
BATCH_POINTS = (1, 63, 64, 65, 96, 256, 257, 1024)
DIMER_SHIFT = (34.0, 60.0, 0.0)           # the copy is turned by 180 degrees about z and moved by this: chain B, in contact with chain A
_CHUNK = 1 << 21                          # point tests per chunk of pairs


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def sphere(n):
    """the golden spiral in NumPy / libm: the formula of th_sasa_sphere.  The tests take their points from th_sasa_sphere itself and
    compare this against it within a few ulp only — nothing is compared as bytes across two libm's"""
    k = np.arange(n, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / float(n)
    rho = np.sqrt(1.0 - z * z)
    phi = k * (math.pi * (3.0 - math.sqrt(5.0)))
    return np.stack([rho * np.cos(phi), rho * np.sin(phi), z], axis=1)


def read_atoms(path=UBQ):
    """every ATOM / HETATM record of the first model, from the fixed columns: a list of dicts (record, name, residue, chain, number,
    xyz, element), the first alternate location of an atom name within a residue only"""
    atoms, seen = [], set()
    with gzip.open(path, "rt") as f:
        for line in f:
            if line[:6] == "ENDMDL":
                break
            if line[:6] not in ("ATOM  ", "HETATM"):
                continue
            name, key = line[12:16].strip(), (line[21], line[22:27], line[17:20])
            if (key, name) in seen:
                continue
            seen.add((key, name))
            element = line[76:78].strip().upper() if len(line) >= 78 else ""
            if not element or not element[0].isalpha():
                element = name.lstrip("0123456789 ").upper()[:1]
            atoms.append(dict(record=line[:6], name=name, residue=line[17:20].strip(), chain=line[21].strip() or "A", number=line[22:27].strip(),
                              xyz=[float(line[30:38]), float(line[38:46]), float(line[46:54])], element=element))
    return atoms


def ubq_atoms(ligand=False):
    """(xyz [n, 3], radius [n], group [n] int32, polar [n] bool, backbone [n] bool, residue names) of 1ubq's heavy polymer atoms in file
    order; ``ligand``: followed by a pseudo-ligand of three atoms S, O, O on the file's first three water sites (group -1)"""
    atoms = [a for a in read_atoms() if a["element"] != "H"]
    polymer = [a for a in atoms if a["record"] == "ATOM  "]
    keys, names = {}, []
    for a in polymer:
        key = (a["chain"], a["number"], a["residue"])
        if key not in keys:
            keys[key] = len(keys)
            names.append(a["residue"])
    rows = [(a["xyz"], RADII.get(a["element"], OTHER_RADIUS), keys[(a["chain"], a["number"], a["residue"])], a["element"] in ("N", "O"),
             a["name"] in ("N", "CA", "C", "O")) for a in polymer]
    if ligand:
        waters = [a for a in atoms if a["record"] == "HETATM" and a["residue"] in WATERS][:3]
        rows += [(a["xyz"], RADII[el], -1, el == "O", False) for a, el in zip(waters, ("S", "O", "O"))]
    return (np.array([r[0] for r in rows], dtype=np.float64), np.array([r[1] for r in rows], dtype=np.float64),
            np.array([r[2] for r in rows], dtype=np.int32), np.array([r[3] for r in rows], dtype=bool),
            np.array([r[4] for r in rows], dtype=bool), names)


def moved_copy(xyz):
    """the rigid motion of the dimer's chain B: (x, y, z) -> (-x + 34, -y + 60, z), rounded to the three decimals of a PDB file"""
    moved = np.stack([-xyz[:, 0] + DIMER_SHIFT[0], -xyz[:, 1] + DIMER_SHIFT[1], xyz[:, 2] + DIMER_SHIFT[2]], axis=1)
    return np.array([[float("%.3f" % v) for v in row] for row in moved.tolist()], dtype=np.float64)


def cases(points_96, points_960):
    """{name: (xyz, radius, probe, points)}: the cases of the rule's write-up.  The points are the caller's (th_sasa_sphere's)"""
    xyz, radius = ubq_atoms()[:2]
    het = ubq_atoms(ligand=True)
    tie_points = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])
    origin = [0.0, 0.0, 0.0]
    return {
        "ubq": (xyz, radius, PROBE, points_96),
        "ubq_960": (xyz, radius, PROBE, points_960),
        "ubq_probe0": (xyz, radius, 0.0, points_96),
        "ubq_dimer": (np.concatenate([xyz, moved_copy(xyz)]), np.concatenate([radius, radius]), PROBE, points_96),
        "ubq_hetero": (het[0], het[1], PROBE, points_96),
        "lone": (np.array([[1.0, 2.0, 3.0]]), np.array([1.7]), PROBE, points_96),
        "pair_3": (np.array([origin, [0.0, 0.0, 3.0]]), np.array([1.5, 1.5]), 1.5, points_96),
        "pair_6": (np.array([origin, [0.0, 0.0, 6.0]]), np.array([1.5, 1.5]), 1.5, points_96),
        "inside": (np.array([origin, [0.5, 0.0, 0.0]]), np.array([1.0, 3.0]), 1.0, points_96),
        "tie": (np.array([origin, [0.0, 0.0, 5.0]]), np.array([2.0, 1.0]), 1.0, tie_points),
        "tie_near": (np.array([origin, [0.0, 0.0, 4.9375]]), np.array([2.0, 1.0]), 1.0, tie_points),
    }


def box_atoms(n, rng, side=14.0):
    """``n`` atoms at seeded random places of a cube of ``side`` Angstrom with radii drawn from the element table"""
    table = np.array(sorted(set(RADII.values())))
    return rng.random((n, 3)) * side, table[rng.integers(0, len(table), n)]


def length_batch(seed=11, lengths=BATCH_LENGTHS):
    """[(xyz, radius)]: the first n atoms of 1ubq for every length, then n atoms of a seeded random 14 Angstrom box for every length"""
    xyz, radius = ubq_atoms()[:2]
    rng = np.random.default_rng(seed)
    return [(xyz[:n], radius[:n]) for n in lengths] + [box_atoms(n, rng) for n in lengths]


def flatten(parts):
    """(xyz [total, 3], radius [total], offsets [S + 1]) of a list of (xyz, radius, ...)"""
    offsets = np.zeros(len(parts) + 1, np.int64)
    np.cumsum([len(p[0]) for p in parts], out=offsets[1:])
    if not parts:
        return np.zeros((0, 3)), np.zeros(0), offsets
    return (np.concatenate([np.asarray(p[0], np.float64).reshape(-1, 3) for p in parts]),
            np.concatenate([np.asarray(p[1], np.float64).reshape(-1) for p in parts]), offsets)


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
def near_pairs(xyz, R, valid):
    """(i, j, s, ties) of every ordered pair with near(i, j), sorted by i then j, with its squared distance s; ties: pairs with
    s == t*t exactly (not near)"""
    n = len(xyz)
    ii, jj, ss, ties = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0)], 0
    with np.errstate(all="ignore"):
        for lo in range(0, n, 1024):
            hi = min(lo + 1024, n)
            dx, dy, dz = (xyz[None, :, c] - xyz[lo:hi, None, c] for c in range(3))
            s = (dx * dx + dy * dy) + dz * dz
            t = R[lo:hi, None] + R[None, :]
            tt = t * t
            both = valid[lo:hi, None] & valid[None, :] & (np.arange(lo, hi)[:, None] != np.arange(n)[None, :])
            ties += int((both & (s == tt)).sum())
            i, j = np.nonzero(both & (s < tt))
            ii.append(i + lo)
            jj.append(j)
            ss.append(s[i, j])
    return np.concatenate(ii), np.concatenate(jj), np.concatenate(ss), ties


def restate(xyz, radius, probe, points, every_pair=False):
    """One structure.  A dict: ``exposed`` int32 [n], ``mask`` uint64 [n, ceil(P / 64)], ``totals`` int64 [3], ``n_near`` [n] and the
    number of ``ties`` (s == t*t between valid atoms, or a tested point exactly on a neighbour's sphere).

    A point is buried iff SOME near atom holds it: the neighbours of every atom are visited nearest first, eight at a time, and an atom
    whose points are all buried is not visited again — which, the result being an AND, changes nothing but the time.
    ``every_pair``: visit them all nevertheless (the count of ties is then complete)."""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    radius = np.asarray(radius, np.float64).reshape(-1)
    points = np.asarray(points, np.float64).reshape(-1, 3)
    n, P = len(xyz), len(points)
    words = (P + 63) // 64
    with np.errstate(all="ignore"):
        R = radius + np.float64(probe)
        valid = np.isfinite(xyz).all(axis=1) & np.isfinite(R) & (R > 0.0)
        i, j, s, ties = near_pairs(xyz, R, valid)
        n_near = np.bincount(i, minlength=n)
        order = np.lexsort((s, i))
        i, j = i[order], j[order]
        rank = np.arange(len(i)) - np.searchsorted(i, i)          # 0 for the nearest neighbour of an atom
        RR = R * R
        buried = np.zeros((n, P), bool)
        step = max(1, _CHUNK // P)
        for r0 in range(0, int(rank.max()) + 1 if len(rank) else 0, 8):
            chosen = (rank >= r0) & (rank < r0 + 8)
            if not every_pair:
                chosen &= ~buried.all(axis=1)[i]
            ci, cj = i[chosen], j[chosen]
            for lo in range(0, len(ci), step):
                a, b = ci[lo:lo + step], cj[lo:lo + step]
                px = xyz[a, 0, None] + R[a, None] * points[None, :, 0]
                py = xyz[a, 1, None] + R[a, None] * points[None, :, 1]
                pz = xyz[a, 2, None] + R[a, None] * points[None, :, 2]
                ex, ey, ez = px - xyz[b, 0, None], py - xyz[b, 1, None], pz - xyz[b, 2, None]
                d = (ex * ex + ey * ey) + ez * ez
                ties += int((d == RR[b, None]).sum())
                inside = d < RR[b, None]
                starts = np.nonzero(np.r_[True, a[1:] != a[:-1]])[0]
                buried[a[starts]] |= np.logical_or.reduceat(inside, starts, axis=0)
    open_ = ~buried & valid[:, None]
    exposed = np.where(valid, open_.sum(axis=1), -1).astype(np.int32)
    padded = np.zeros((n, words * 64), bool)
    padded[:, :P] = open_
    weights = np.uint64(1) << np.arange(64, dtype=np.uint64)
    mask = (padded.reshape(n, words, 64).astype(np.uint64) * weights).sum(axis=2, dtype=np.uint64)
    totals = np.array([valid.sum(), (exposed == 0).sum(), exposed[valid].sum()], dtype=np.int64)
    return dict(exposed=exposed, mask=mask, totals=totals, n_near=n_near, ties=ties, valid=valid)


def restate_batch(xyz, radius, offsets, probe, points):
    """(exposed [total], mask [total, words], totals [S, 3]) of a flat batch: every structure on its own"""
    points = np.asarray(points, np.float64).reshape(-1, 3)
    words = (len(points) + 63) // 64
    exposed, mask, totals = [np.zeros(0, np.int32)], [np.zeros((0, words), np.uint64)], []
    for a, b in zip(offsets[:-1], offsets[1:]):
        one = restate(xyz[a:b], radius[a:b], probe, points)
        exposed.append(one["exposed"])
        mask.append(one["mask"])
        totals.append(one["totals"])
    return np.concatenate(exposed), np.concatenate(mask), np.array(totals, dtype=np.int64).reshape(-1, 3)


def atom_areas(exposed, radius, probe, n_points):
    """area_i = exposed_i * (4 pi R_i R_i / n_points), multiplied left to right; 0 for an invalid atom"""
    R = np.asarray(radius, np.float64) + np.float64(probe)
    unit = 4.0 * math.pi * R * R / float(n_points)
    return np.where(exposed >= 0, exposed.astype(np.float64) * unit, 0.0)


def residue_areas(area, group, polar, backbone, n_residues):
    """float64 [4, residues]: the sequential sums over the atoms in file order of all, polar, apolar and backbone areas; and the three
    totals (all, polar, apolar) over every atom"""
    sums, totals = np.zeros((4, n_residues)), [0.0, 0.0, 0.0]
    for a, g, p, b in zip(area.tolist(), group.tolist(), polar.tolist(), backbone.tolist()):
        totals[0] += a
        totals[1 if p else 2] += a
        if g < 0:
            continue
        sums[0, g] += a
        sums[1 if p else 2, g] += a
        if b:
            sums[3, g] += a
    return sums, np.array(totals)


def burial(rsa, core=0.2, surface=0.5):
    return [-1 if v != v else 0 if v < core else 2 if v >= surface else 1 for v in np.asarray(rsa).tolist()]


def golden_arrays(points_96, points_960):
    """the arrays of tests/golden/sasa_golden.npz"""
    inputs = cases(points_96, points_960)
    out = {"cases": np.array(CASES), "points_96": points_96, "points_960": points_960, "points_tie": inputs["tie"][3]}
    for name in CASES:
        xyz, radius, probe, points = inputs[name]
        one = restate(xyz, radius, probe, points)
        out[f"{name}_exposed"], out[f"{name}_mask"], out[f"{name}_totals"] = one["exposed"], one["mask"], one["totals"]
    _, _, group, polar, backbone, names = ubq_atoms()
    het = ubq_atoms(ligand=True)
    layouts = {"ubq": (group, polar, backbone, 76), "ubq_960": (group, polar, backbone, 76), "ubq_probe0": (group, polar, backbone, 76),
               "ubq_dimer": (np.concatenate([group, group + 76]), np.concatenate([polar, polar]), np.concatenate([backbone, backbone]), 152),
               "ubq_hetero": (het[2], het[3], het[4], 76)}
    for name, (g, p, b, n_res) in layouts.items():
        xyz, radius, probe, points = inputs[name]
        area = atom_areas(out[f"{name}_exposed"], radius, probe, len(points))
        out[f"{name}_residue_area"], out[f"{name}_area"] = residue_areas(area, g, p, b, n_res)
    # the interface of the dimer: each chain alone (chain A alone is ubq) minus the complex
    xyz, radius, probe, points = inputs["ubq_dimer"]
    alone = restate(xyz[602:], radius[602:], probe, points)
    area_b = atom_areas(alone["exposed"], radius[602:], probe, len(points))
    sums_b, totals_b = residue_areas(area_b, group, polar, backbone, 76)
    separate = np.concatenate([out["ubq_residue_area"][0], sums_b[0]])
    out["ubq_dimer_area_lost"] = separate - out["ubq_dimer_residue_area"][0]
    out["ubq_dimer_interface"] = np.array((0.0 + out["ubq_area"][0] + totals_b[0]) - out["ubq_dimer_area"][0])
    return out
