"""NumPy restatement of th_secondary_structure (include/timed_hip.h): the DSSP rule (Kabsch & Sander 1983) on the backbone atoms of
one structure at a time — hydrogen bonds by the electrostatic energy, then turns, helices, bridges, ladders and bends as integer
pattern matching.  Plain NumPy and loops; every float64 product, sum, square root and division is one NumPy operation, so each is
rounded on its own.  Computed by this file, NOT by mkdssp, PyMOL's dss or STRIDE, none of which is available: the rule is this
project's reading of the published definition (PARITY UNPINNED AGAINST DSSP).

Also the inputs of the tests: the backbone of tests/golden/1ubq.pdb1.gz read from the fixed columns of its ATOM records (no timed_hip
involved), the NeRF builder of ideal backbones, and the tiled copies of 1ubq of the length batch."""
import gzip
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
UBQ = os.path.join(HERE, "golden", "1ubq.pdb1.gz")
GOLDEN = os.path.join(HERE, "golden", "secstruct_golden.npz")
LETTERS = "-HBEGITS"
THREE = "CHEEHHCC"                   # three-state letter of each code: H, G, I -> H; E, B -> E; the rest -> C
COS_70 = 0.3420201433256688
F_TURN3, F_TURN4, F_TURN5, F_BEND, F_PARALLEL, F_ANTIPARALLEL, F_CONN, F_VALID = (1 << b for b in range(8))
UBQ_STRING = "-EEEEEETTS-EEEEE--TTSBHHHHHHHHHHHH---GGGEEEEETTEE--TTSBTGGGT--TT-EEEEEE--S--"
# name -> (phi, psi, residues, expected string)
IDEAL = {"alpha": (-57.8, -47.0, 20, "-HHHHHHHHHHHHHHHHHH-"), "three10": (-49.0, -26.0, 12, "-GGGGGGGGGG-"),
         "pi": (-57.1, -69.7, 14, "-IIIIIIIIIIII-"), "beta": (-120.0, 130.0, 12, "-" * 12)}
CASES = ("ubq", "ubq_cut", "alpha", "three10", "pi", "beta", "two_chains", "missing_o")
STRINGS = {"ubq": UBQ_STRING, "ubq_cut": UBQ_STRING[:29] + "-" + UBQ_STRING[36:], "two_chains": "-HHHHHHHH--HHHHHHHH-", "missing_o": "-HHHHH---HHHHHHHHHH-"}
STRINGS.update({name: v[3] for name, v in IDEAL.items()})
BATCH_LENGTHS = (0, 1, 2, 4, 5, 6, 63, 64, 65, 128, 129, 256, 257, 300)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def ubq_backbone():
    """([76, 4, 3] N, CA, C, O; chain [76] int32 zeros; no_h [76] uint8, 1 for PRO) of 1ubq, from the fixed columns"""
    rows, order = {}, []
    with gzip.open(UBQ, "rt") as f:
        for line in f:
            if line[:6] != "ATOM  ":
                continue
            key = (line[21], line[22:27])
            if key not in rows:
                rows[key] = {"name": line[17:20].strip()}
                order.append(key)
            rows[key].setdefault(line[12:16].strip(), [float(line[30:38]), float(line[38:46]), float(line[46:54])])
    nan = [np.nan] * 3
    backbone = np.array([[rows[k].get(a, nan) for a in ("N", "CA", "C", "O")] for k in order], dtype=np.float64)
    no_h = np.array([rows[k]["name"] == "PRO" for k in order], dtype=np.uint8)
    return backbone, np.zeros(len(order), np.int32), no_h


def _place(a, b, c, bond, angle, torsion):
    """NeRF: the point at ``bond`` from c, making ``angle`` (degrees) with b-c and ``torsion`` (degrees) with a-b-c"""
    angle, torsion = np.radians(angle), np.radians(torsion)
    bc = (c - b) / np.linalg.norm(c - b)
    n = np.cross(b - a, bc)
    n /= np.linalg.norm(n)
    m = np.cross(n, bc)
    d = np.array([-bond * np.cos(angle), bond * np.sin(angle) * np.cos(torsion), bond * np.sin(angle) * np.sin(torsion)])
    return c + d[0] * bc + d[1] * m + d[2] * n


def ideal_backbone(phi, psi, n):
    """[n, 4, 3] of an ideal backbone: N-CA 1.458, CA-C 1.525, C-N 1.329, C=O 1.231; N-CA-C 111.0, CA-C-N 116.2, C-N-CA 121.7,
    CA-C-O 120.5 degrees; omega 180; O opposite the next N (torsion psi + 180)"""
    out = np.zeros((n, 4, 3))
    out[0, 0] = (0.0, 0.0, 0.0)
    out[0, 1] = (1.458, 0.0, 0.0)
    out[0, 2] = out[0, 1] + 1.525 * np.array([-np.cos(np.radians(111.0)), np.sin(np.radians(111.0)), 0.0])
    for i in range(n):
        N, CA, C = out[i, 0], out[i, 1], out[i, 2]
        out[i, 3] = _place(N, CA, C, 1.231, 120.5, psi + 180.0)
        if i + 1 < n:
            out[i + 1, 0] = _place(N, CA, C, 1.329, 116.2, psi)
            out[i + 1, 1] = _place(CA, C, out[i + 1, 0], 1.458, 121.7, 180.0)
            out[i + 1, 2] = _place(C, out[i + 1, 0], out[i + 1, 1], 1.525, 111.0, phi)
    return out


def cases():
    """{name: (backbone, chain, no_h)}: the cases of the rule's write-up"""
    ubq = ubq_backbone()
    keep = np.r_[0:30, 36:76]                                 # residues 30 .. 35 (counted from 0, as the rule counts) removed
    out = {"ubq": ubq, "ubq_cut": tuple(a[keep] for a in ubq)}
    for name, (phi, psi, n, _) in IDEAL.items():
        out[name] = (ideal_backbone(phi, psi, n), np.zeros(n, np.int32), np.zeros(n, np.uint8))
    alpha = out["alpha"][0]
    out["two_chains"] = (alpha, np.array([0] * 10 + [1] * 10, np.int32), np.zeros(20, np.uint8))
    holed = alpha.copy()
    holed[7, 3] = np.nan
    out["missing_o"] = (holed, np.zeros(20, np.int32), np.zeros(20, np.uint8))
    return out


def tiled_ubq(length, rng, sigma=0.2, shift=40.0):
    """``length`` residues of copies of 1ubq's backbone with seeded noise, copy k shifted k * ``shift`` Angstrom along x under chain
    id k, truncated"""
    backbone, _, no_h = ubq_backbone()
    copies = -(-length // len(backbone)) if length else 0
    parts = [backbone + rng.normal(0.0, sigma, backbone.shape) + np.array([k * shift, 0.0, 0.0]) for k in range(copies)]
    bb = np.concatenate(parts)[:length] if parts else np.zeros((0, 4, 3))
    chain = np.repeat(np.arange(copies, dtype=np.int32), len(backbone))[:length]
    return bb, chain.astype(np.int32), np.tile(no_h, copies)[:length].astype(np.uint8)


def length_batch(seed=7, lengths=BATCH_LENGTHS):
    rng = np.random.default_rng(seed)
    return [tiled_ubq(n, rng) for n in lengths]


def flatten(parts):
    """(backbone [total, 4, 3], chain, no_h, offsets [S + 1]) of a list of (backbone, chain, no_h)"""
    offsets = np.zeros(len(parts) + 1, np.int64)
    np.cumsum([len(p[0]) for p in parts], out=offsets[1:])
    if not parts:
        return np.zeros((0, 4, 3)), np.zeros(0, np.int32), np.zeros(0, np.uint8), offsets
    return (np.concatenate([np.asarray(p[0], np.float64).reshape(-1, 4, 3) for p in parts]), np.concatenate([p[1] for p in parts]).astype(np.int32),
            np.concatenate([p[2] for p in parts]).astype(np.uint8), offsets)


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
def _dist(a, b):
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return np.sqrt((dx * dx + dy * dy) + dz * dz)


def prepare(backbone, chain, no_h):
    """valid [L], conn [L] (link i -> i + 1; false at L - 1), H [L, 3] (NaN where there is none), has_h [L]"""
    L = len(backbone)
    valid = np.isfinite(backbone.reshape(L, 12)).all(axis=1)
    conn = np.zeros(L, bool)
    H = np.full((L, 3), np.nan)
    has_h = np.zeros(L, bool)
    with np.errstate(all="ignore"):
        for i in range(L - 1):
            if valid[i] and valid[i + 1] and chain[i] == chain[i + 1]:
                d = backbone[i, 2] - backbone[i + 1, 0]
                conn[i] = bool((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] <= 6.25)
        for i in range(1, L):
            if conn[i - 1] and not no_h[i]:
                v = backbone[i - 1, 2] - backbone[i - 1, 3]
                norm = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
                h = backbone[i, 0] + v / norm
                if np.isfinite(h).all():
                    H[i], has_h[i] = h, True
    return valid, conn, H, has_h


def energies(backbone, valid, H, has_h):
    """e [L, L] int32 in milli-kcal/mol (acceptor, donor) and the mask of the pairs whose energy is taken"""
    L = len(backbone)
    N, CA, C, O = (backbone[:, k] for k in range(4))
    idx = np.arange(L)
    with np.errstate(all="ignore"):
        dca = CA[:, None] - CA[None, :]
        near = (dca[..., 0] * dca[..., 0] + dca[..., 1] * dca[..., 1]) + dca[..., 2] * dca[..., 2] < 81.0
        taken = valid[:, None] & has_h[None, :] & (idx[None, :] != idx[:, None]) & (idx[None, :] != idx[:, None] + 1) & near
        a, d = np.nonzero(taken)
        r_on, r_ch, r_oh, r_cn = _dist(O[a], N[d]), _dist(C[a], H[d]), _dist(O[a], H[d]), _dist(C[a], N[d])
        q = ((1.0 / r_on + 1.0 / r_ch) - 1.0 / r_oh) - 1.0 / r_cn
        close = (r_on < 0.5) | (r_ch < 0.5) | (r_oh < 0.5) | (r_cn < 0.5)
        ev = np.floor((27.888 * q) * 1000.0 + 0.5)
        ev = np.where(close | (ev < -9900.0), -9900.0, ev)
    assert np.isfinite(ev).all()
    e = np.zeros((L, L), np.int32)
    e[a, d] = ev.astype(np.int32)
    return e, taken


def restate(backbone, chain, no_h):
    """The rule on one structure.  Returns a dict: ``cls`` [L] uint8, ``residue`` [L, 6] int32, ``totals`` [10] int64, ``bits``
    [L * ceil(L / 64)] uint64 (row = acceptor, bit = donor) and ``hb`` [L, L] bool."""
    backbone = np.asarray(backbone, np.float64).reshape(-1, 4, 3)
    L = len(backbone)
    chain, no_h = np.asarray(chain).reshape(-1), np.asarray(no_h).reshape(-1)
    assert len(chain) == L and len(no_h) == L
    W = (L + 63) // 64
    valid, conn, H, has_h = prepare(backbone, chain, no_h)
    e, taken = energies(backbone, valid, H, has_h)
    hb = taken & (e < -500)

    def bond(a, d):
        return 0 <= a < L and 0 <= d < L and bool(hb[a, d])

    def link(i):
        return 0 <= i < L and bool(conn[i])

    def turn(i, n):
        return bond(i, i + n) and all(link(k) for k in range(i, i + n))

    def framed(i, j):
        return abs(i - j) >= 3 and link(i - 1) and link(i) and link(j - 1) and link(j)

    def parallel(i, j):
        return framed(i, j) and ((bond(i - 1, j) and bond(j, i + 1)) or (bond(j - 1, i) and bond(i, j + 1)))

    def antiparallel(i, j):
        return framed(i, j) and ((bond(i, j) and bond(j, i)) or (bond(i - 1, j + 1) and bond(j - 1, i + 1)))

    cls = np.zeros(L, np.uint8)
    residue = np.zeros((L, 6), np.int32)
    residue[:, :2] = -1
    for i in range(L):
        flags = (F_VALID if valid[i] else 0) | (F_CONN if conn[i] else 0)
        for b, n in enumerate((3, 4, 5)):
            flags |= (1 << b) if turn(i, n) else 0
        helix = {n: any(turn(k - 1, n) and turn(k, n) for k in range(i - n + 1, i + 1)) for n in (3, 4, 5)}
        inside = any(turn(k, n) for n in (3, 4, 5) for k in range(i - n + 1, i))
        partners, ladder = [], False
        if link(i - 1) and link(i):
            for j in range(L):
                p, a = parallel(i, j), antiparallel(i, j)
                if not (p or a):
                    continue
                partners.append(j)
                flags |= (F_PARALLEL if p else 0) | (F_ANTIPARALLEL if a else 0)
                ladder |= p and (parallel(i + 1, j + 1) or parallel(i - 1, j - 1))
                ladder |= a and (antiparallel(i + 1, j - 1) or antiparallel(i - 1, j + 1))
        if link(i - 2) and link(i - 1) and link(i) and link(i + 1):
            a, b = backbone[i, 1] - backbone[i - 2, 1], backbone[i + 2, 1] - backbone[i, 1]
            with np.errstate(all="ignore"):
                dot = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
                na, nb = np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]), np.sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2])
                flags |= F_BEND if dot / (na * nb) < COS_70 else 0
        code = (1 if helix[4] else 3 if ladder else 2 if partners else 4 if helix[3] else 5 if helix[5] else 6 if inside else 7 if flags & F_BEND else 0)
        cls[i] = code if valid[i] else 0
        residue[i] = (partners[0] if partners else -1, partners[1] if len(partners) > 1 else -1, flags, int(hb[i].sum()), int(hb[:, i].sum()), len(partners))
    bits = np.zeros((L, W), np.uint64)
    for a, d in zip(*np.nonzero(hb)):
        bits[a, d // 64] |= np.uint64(1) << np.uint64(d % 64)
    totals = np.array([int(valid.sum()), int(hb.sum())] + np.bincount(cls, minlength=8).tolist(), np.int64)
    return dict(cls=cls, residue=residue, totals=totals, bits=bits.reshape(-1), hb=hb, energy=e, taken=taken)


def restate_batch(backbone, chain, no_h, offsets):
    """the tables th_secondary_structure returns for a flat batch: (class [total] uint8, residue [total, 6] int32, structure [S, 10]
    int64, bits [sum L * ceil(L / 64)] uint64)"""
    backbone = np.asarray(backbone, np.float64).reshape(-1, 4, 3)
    offsets = np.asarray(offsets, np.int64).reshape(-1)
    parts = [restate(backbone[lo:hi], chain[lo:hi], no_h[lo:hi]) for lo, hi in zip(offsets[:-1], offsets[1:])]
    if not parts:
        return np.zeros(0, np.uint8), np.zeros((0, 6), np.int32), np.zeros((0, 10), np.int64), np.zeros(0, np.uint64)
    return (np.concatenate([p["cls"] for p in parts]), np.concatenate([p["residue"] for p in parts]), np.stack([p["totals"] for p in parts]),
            np.concatenate([p["bits"] for p in parts]))


def as_string(cls):
    return "".join(LETTERS[c] for c in np.asarray(cls).tolist())


def golden_arrays(inputs=None):
    """what tests/golden/secstruct_golden.npz holds: per case its class codes, residue table, totals and bond bitmap"""
    inputs = inputs or cases()
    out = {"cases": np.array(CASES)}
    for name in CASES:
        res = restate(*inputs[name])
        for key in ("cls", "residue", "totals", "bits"):
            out[f"{name}_{key}"] = res[key]
    return out
