"""NumPy restatement of th_packing_density (include/timed_hip.h) and the seeded synthetic structures of the packing-density
tests.  The restatement keeps the reference's float64 operation order — np.sqrt(((dx*dx + dy*dy) + dz*dz)) < radius, which is what
np.square(xyz - xyz[i]).sum(axis=1) evaluates for three columns — vectorised over blocks of atoms i; tests/test_packdensity_host.py
holds it to tests/golden/packdensity_golden.npz (the reference's own output) byte for byte, the GPU tests use it for random cases.

A synthetic structure is a list of chains, a chain a list of residues, a residue a dict(name, hetero, atoms=[(atom name, element,
xyz)]).  golden_structure(name) rebuilds one from its seed; the fixture records the sha256 of its coordinates."""
import hashlib

import numpy as np

RADII = (7.0, 4.5, 6.3)                 # 6.3 is not representable in binary; 4.5 and 7 are
FILTERS = ("all", "backbone", "ca")     # the reference's three
TILE = 256                              # atoms per workgroup tile of k_contacts

# offsets of nominal length exactly r, on three-decimal coordinates: axis-aligned and Pythagorean ((2, 3, 6) has length 7)
TIE_OFFSETS = {
    7.0: [(7, 0, 0), (0, -7, 0), (0, 0, 7), (2, 3, 6), (-6, 2, 3), (3, -6, 2), (6, 3, -2)],
    4.5: [(4.5, 0, 0), (0, 0, -4.5), (1.5, 3, 3), (-3, 1.5, 3), (3, 3, -1.5)],
    6.3: [(6.3, 0, 0), (0, 6.3, 0), (1.8, 2.7, 5.4), (-5.4, 1.8, 2.7), (2.7, -5.4, 1.8)],
}

# name -> (seed, heavy atoms, chains, planted)
GOLDEN_CASES = {
    "n0": (10, 0, 1, False),
    "n1": (11, 1, 1, False),
    "n2": (12, 2, 1, False),
    "n255": (13, TILE - 1, 1, False),
    "n256": (14, TILE, 1, False),
    "n257": (15, TILE + 1, 2, False),
    "n513": (16, 2 * TILE + 1, 2, True),
    "mix": (17, 900, 3, True),
}

_NAMES = ("N", "CA", "C", "O", "CB", "CG", "CD", "NE", "CZ", "OXT")


def restate_density(xyz, offsets, radius):
    """int32 [total]: contact number of every atom within its own structure"""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    out = np.empty(len(xyz), np.int32)
    r = np.float64(radius)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(len(offsets) - 1):
            lo, hi = int(offsets[s]), int(offsets[s + 1])
            a = xyz[lo:hi]
            block = max(1, min(512, 4_000_000 // max(hi - lo, 1)))      # about 100 MB of differences at a time
            for b in range(lo, hi, block):
                d = a[None, :, :] - xyz[b:min(hi, b + block), None, :]
                q = np.square(d)
                dist = np.sqrt((q[..., 0] + q[..., 1]) + q[..., 2])
                out[b:min(hi, b + block)] = (dist < r).sum(axis=1) - 1
    return out


def restate_residues(density, group, selected, n_groups):
    """float64 [n_groups]: the running half-average of th_packing_density over the selected atoms of each residue in index order"""
    out = np.full(n_groups, -1.0)
    for i in range(len(density)):
        g = int(group[i])
        if g < 0 or not selected[i]:
            continue
        d = np.float64(density[i])
        out[g] = d if out[g] == -1.0 else (out[g] + d) / 2
    return out


def selects(name, atom_filter):
    if atom_filter == "all":
        return True
    if atom_filter == "backbone":
        return name in ("N", "CA", "C", "O")
    if atom_filter == "ca":
        return name in "CA"                # substring, as the reference
    if atom_filter == "calpha":
        return name == "CA"
    raise ValueError(atom_filter)


def golden_structure(name):
    seed, n_heavy, n_chains, planted = GOLDEN_CASES[name]
    return build_structure(seed, n_heavy, n_chains, planted)


def build_structure(seed, n_heavy, n_chains=1, planted=False, finite_only=False):
    """n_heavy non-hydrogen atoms at three-decimal coordinates in a box of protein-like density, in residues of 1..10 atoms (some
    without backbone atoms, some with a hydrogen named H, one of hydrogens only), spread over n_chains chains (the last chain is
    hetero when there are three).  planted: pairs at nominal distance exactly r for every r of RADII, duplicated coordinates and —
    unless finite_only — one atom with a NaN and one with an infinite coordinate, the NaN on a CA that leads its residue's "ca"
    selection."""
    rng = np.random.default_rng(seed)
    half = max(3.0, (n_heavy * 20.0) ** (1 / 3) / 2)
    coords = np.round(rng.uniform(-half, half, (n_heavy, 3)), 3)
    if planted:
        slots = rng.permutation(n_heavy)
        at = 0
        for r in RADII:
            for off in TIE_OFFSETS[r]:
                a, b = slots[at], slots[at + 1]
                at += 2
                coords[b] = np.round(coords[a] + np.array(off, dtype=np.float64), 3)
        for _ in range(4):                                  # duplicates, one of them three atoms deep
            a, b = slots[at], slots[at + 1]
            at += 2
            coords[b] = coords[a]
        coords[slots[at]] = coords[slots[at - 1]]
        at += 1
    chains = [[] for _ in range(n_chains)]
    i, resno = 0, 0
    bounds = [int(round(n_heavy * (c + 1) / n_chains)) for c in range(n_chains)]
    nan_done = inf_done = finite_only or not planted
    while i < n_heavy:
        c = next(k for k, b in enumerate(bounds) if i < b)
        kind = rng.integers(0, 8)
        size = int(min(rng.integers(1, 11), bounds[c] - i))
        names = _NAMES[4:4 + size] if kind == 0 and size <= 6 else _NAMES[:size]       # kind 0: side-chain atoms only
        atoms = []
        for k, nm in enumerate(names):
            if k == 1 and kind in (1, 2):
                atoms.append(("H", "H", np.round(rng.uniform(-half, half, 3), 3)))
            atoms.append((nm, nm[0], coords[i].copy()))
            i += 1
        if "CA" in names and size >= 4 and not nan_done and c == 0:
            atoms[[a[0] for a in atoms].index("CA")][2][1] = np.nan
            nan_done = True
        elif size >= 3 and not inf_done and c == 0:
            atoms[0][2][2] = np.inf
            inf_done = True
        resno += 1
        chains[c].append(dict(name="GLY" if size <= 4 else "LYS", number=resno, hetero=n_chains == 3 and c == 2, atoms=atoms))
        if kind == 3:                                       # a residue of hydrogens only: no selected atom under any filter
            resno += 1
            chains[c].append(dict(name="HOH", number=resno, hetero=n_chains == 3 and c == 2,
                                  atoms=[("H", "H", np.round(rng.uniform(-half, half, 3), 3))]))
    return chains


def flatten(chains, atom_filter, reported_chain=0):
    """(xyz [n, 3], group [n], selected [n], n_groups) over the non-hydrogen atoms, chain after chain; the residues of
    ``reported_chain`` are the groups"""
    xyz, group, selected = [], [], []
    n_groups = 0
    for c, chain in enumerate(chains):
        for res in chain:
            g = -1
            if c == reported_chain:
                g = n_groups
                n_groups += 1
            for nm, el, pos in res["atoms"]:
                if el == "H":
                    continue
                xyz.append(pos)
                group.append(g)
                selected.append(1 if g >= 0 and selects(nm, atom_filter) else 0)
    return (np.array(xyz, dtype=np.float64).reshape(-1, 3), np.array(group, dtype=np.int32), np.array(selected, dtype=np.uint8), n_groups)


def coords_sha256(chains):
    xyz = flatten(chains, "all")[0]
    return hashlib.sha256(np.ascontiguousarray(xyz).tobytes()).hexdigest()


def write_pdb(chains, path):
    """fixed-column PDB text of a synthetic structure with finite coordinates; chains are A, B, C; the B-factor of every atom of a
    residue is 10 + number / 4 (exact in two decimals)"""
    lines, serial = [], 0
    for c, chain in enumerate(chains):
        for res in chain:
            rec = "HETATM" if res["hetero"] else "ATOM  "
            for nm, el, pos in res["atoms"]:
                serial += 1
                padded = nm if len(nm) == 4 else " " + nm.ljust(3)
                lines.append("%s%5d %s %3s %s%4d    %8.3f%8.3f%8.3f%6.2f%6.2f          %2s" % (
                    rec, serial % 100000, padded, res["name"], "ABC"[c], res["number"], pos[0], pos[1], pos[2], 1.0,
                    bfactor_of(res), el))
    with open(path, "w") as f:
        f.write("\n".join(lines + ["END", ""]))


def bfactor_of(res):
    return 10.0 + res["number"] / 4.0
