"""Seeded synthetic structures for the voxeliser tests, and restatements of spec items 3-5 (timed_hip/voxeliser.py) on boolean
frames: the specification itself and two deliberately wrong ones.  Plain helpers, no tests: tests/test_voxel_cases_host.py checks
on the CPU that the generators are sharp (they separate the wrong restatements from the right one), that every cloud fits the
kernel's atom list, and that no weight is small enough for denormal flushing to matter; tests/test_gpu_voxelise_sweep.py runs the
same clouds through th_voxelise against oracle/voxel_oracle.py, tests/test_gpu_voxelise_batch.py through th_voxelise_batch, many to
a launch.  Both entry points run the one kernel of csrc/voxelise.hip (th_voxelise is the one-structure case); the comparison both
test files share (`same`) and the digests of the frames th_voxelise gave while it still had a kernel of its own
(tests/golden/voxelise_digests.json) are at the end of this file.

A cloud is (xyz float32 [n,3], ch int32 [n], sg float32 [n], frt float32 [n_frames,12]) — the four arrays th_voxelise takes, and one
structure of a th_voxelise_batch call.  Every
generator draws its atoms in the LOCAL frame of one residue (targets t), then maps them back with p = CA + R^T t in float64, R and
CA being the float32 values of the frame row, and rounds p to float32: what the kernel reads is a float32 structure whose atoms sit
where the generator wants them to within the rounding of a coordinate tens of Angstrom from the origin (~4e-6)."""
import hashlib
import json
import os
from collections import namedtuple

import numpy as np

Cloud = namedtuple("Cloud", "xyz ch sg frt")
Case = namedtuple("Case", "cloud V edge C")

MAX_LIST = 2048                       # kMaxList of csrc/voxelise.hip, the one kernel of both entry points: encodable atoms inside one frame
CHUNK = 256                           # atoms per pass of the kernel's ordered compaction

# (voxels_per_side, frame_edge_length, n_channels) of the geometry sweep
SWEEP = [(21, 20.0, 6), (21, 21.0, 5), (9, 12.5, 8), (5, 7.3, 8), (3, 2.0, 3), (1, 4.0, 1), (1, 4.0, 2)]


def voxel_edge(V, edge):
    """the kernel's a: float32(edge) / float32(V), as a Python float"""
    return float(np.float32(edge) / np.float32(V))


def rotation(rng):
    """random proper rotation, float64"""
    Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    Q *= np.sign(np.linalg.det(Q))
    return Q


def origin(rng):
    """a CA position 20-60 Angstrom from the origin"""
    v = rng.standard_normal(3)
    return v / np.linalg.norm(v) * rng.uniform(20.0, 60.0)


def frame_row(rng, ca=None):
    return np.concatenate([rotation(rng).reshape(9), origin(rng) if ca is None else np.asarray(ca, np.float64)]).astype(np.float32)


def place(targets, row):
    """p = CA + R^T t in float64 from the float32 frame row, rounded to float32"""
    R, ca = row[:9].astype(np.float64).reshape(3, 3), row[9:].astype(np.float64)
    return (ca[None, :] + np.asarray(targets, np.float64) @ R).astype(np.float32)


def sigmas(rng, n, a):
    """Gaussian widths in [0.26 a, 0.9 a]: never below 0.25 a, so the smallest of an atom's 27 weights is above exp(-54)"""
    return rng.uniform(0.26 * a, 0.9 * a, n).astype(np.float32)


def _cloud(rng, targets, ch, V, edge, ca):
    row = frame_row(rng, ca)
    return Cloud(place(targets, row), np.asarray(ch, np.int32), sigmas(rng, len(ch), voxel_edge(V, edge)), row[None, :])


def merge(*clouds):
    """one structure that holds the atoms of every cloud, and every cloud's frames"""
    return Cloud(*(np.concatenate([getattr(c, f) for c in clouds]) for f in Cloud._fields))


def subset(cloud, keep):
    return Cloud(cloud.xyz[keep], cloud.ch[keep], cloud.sg[keep], cloud.frt)


def face_cloud(V, edge, C, n, seed, ca=None):
    """atoms ON voxel faces: one local axis at (k +- 0.5) a exactly, k from one voxel beyond the cube on one side to one voxel beyond
    it on the other, the other two axes uniform over the cube and a margin of one voxel; channels from [-1, C] inclusive.  Whether
    such an atom rounds into voxel k or its neighbour is decided by the last bit of local / a + 0.5."""
    rng = np.random.default_rng(seed)
    a, centre = voxel_edge(V, edge), V // 2
    half = (centre + 1.5) * a
    t = rng.uniform(-half, half, (n, 3))
    k = rng.integers(-centre - 1, centre + 2, n)
    t[np.arange(n), rng.integers(0, 3, n)] = (k + rng.choice([-0.5, 0.5], n)) * a
    return _cloud(rng, t, rng.integers(-1, C + 1, n), V, edge, ca)


def uniform_cloud(V, edge, C, n, seed, ca=None):
    """atoms uniform over the cube and a margin of one voxel, channels from [-1, C] inclusive"""
    rng = np.random.default_rng(seed)
    half = (V // 2 + 1.5) * voxel_edge(V, edge)
    return _cloud(rng, rng.uniform(-half, half, (n, 3)), rng.integers(-1, C + 1, n), V, edge, ca)


def _in_voxels(rng, vox, V, edge):
    """local targets inside the given voxels [n,3] (indices 0..V-1), at most 0.45 a from the voxel centre on each axis"""
    a = voxel_edge(V, edge)
    return (np.asarray(vox) - V // 2 + rng.uniform(-0.45, 0.45, np.shape(vox))) * a


def interior_cloud(V, edge, C, n, seed, ca=None):
    """every atom's voxel is in [1, V-2] on each axis: its whole 3x3x3 block lies inside the cube.  Channels 0..C-1."""
    assert V >= 3
    rng = np.random.default_rng(seed)
    return _cloud(rng, _in_voxels(rng, rng.integers(1, V - 1, (n, 3)), V, edge), rng.integers(0, C, n), V, edge, ca)


def border_cloud(V, edge, C, n, seed, ca=None):
    """every atom's voxel is on a face, an edge or a corner of the cube (a third of the atoms each).  Channels 0..C-1."""
    rng = np.random.default_rng(seed)
    vox = rng.integers(0, V, (n, 3))
    for i in range(n):
        axes = rng.permutation(3)[:1 + i % 3]                      # 1, 2, 3 axes pinned to an outer layer: face, edge, corner
        vox[i, axes] = rng.choice([0, V - 1], len(axes))
    return _cloud(rng, _in_voxels(rng, vox, V, edge), rng.integers(0, C, n), V, edge, ca)


def stacked_cloud(V, edge, C, n, seed, channel=0, n_voxels=4, ca=None):
    """n atoms of one channel inside the same few voxels"""
    rng = np.random.default_rng(seed)
    few = rng.integers(0, V, (n_voxels, 3))
    return _cloud(rng, _in_voxels(rng, few[rng.integers(0, n_voxels, n)], V, edge), np.full(n, channel), V, edge, ca)


def outside_targets(rng, n, V, edge):
    """local targets at least one voxel beyond the cube on one axis, anywhere within three half-edges on the others"""
    a, centre = voxel_edge(V, edge), V // 2
    t = rng.uniform(-3.0 * (centre + 0.5) * a, 3.0 * (centre + 0.5) * a, (n, 3))
    t[np.arange(n), rng.integers(0, 3, n)] = rng.choice([-1.0, 1.0], n) * rng.uniform((centre + 1.5) * a, 3.0 * (centre + 0.5) * a, n)
    return t


def three_frames(generator, V, edge, C, n, seed):
    """three clouds of n atoms, each with its own rotation and origin, the origins within 0.3 edge of each other on every axis so
    that each frame also sees atoms of the other two at positions nobody chose"""
    base = origin(np.random.default_rng(seed))
    shift = np.random.default_rng(seed + 1).uniform(-0.3 * edge, 0.3 * edge, (3, 3))
    return merge(*(generator(V, edge, C, n, seed + 10 + i, ca=base + shift[i]) for i in range(3)))


# which atoms of each 256-atom chunk lie inside the cube: nothing, one full wave, a sprinkle, a full wave and a sprinkle
CHUNK_PLAN = ("none", "wave", "sparse", "none", "wave+sparse", "sparse", "sparse", "none")


def chunk_plan_mask(n, sparse, seed):
    """bool [n]: the atoms meant to be inside, chunk by chunk after CHUNK_PLAN; `sparse` is the fraction of a sprinkle"""
    rng = np.random.default_rng(seed)
    want = np.zeros(n, bool)
    for c, base in enumerate(range(0, n, CHUNK)):
        plan, m = CHUNK_PLAN[c % len(CHUNK_PLAN)], min(CHUNK, n - base)
        if c == (n - 1) // CHUNK:
            plan = "sparse"                                          # the last, partial chunk always holds some
        if "wave" in plan:
            w = int(rng.integers(0, 4))
            want[base + 64 * w:base + 64 * (w + 1)] = True
        if "sparse" in plan:
            want[base:base + m] |= rng.random(m) < sparse
    return want


def chunked_cloud(V, edge, C, n, sparse, seed):
    """n atoms in one frame; those inside the cube are scattered through the chunks after CHUNK_PLAN, the rest lie outside it"""
    rng = np.random.default_rng(seed)
    want = chunk_plan_mask(n, sparse, seed + 1)
    a, centre = voxel_edge(V, edge), V // 2
    t = outside_targets(rng, n, V, edge)
    t[want] = rng.uniform(-(centre + 0.49) * a, (centre + 0.49) * a, (int(want.sum()), 3))
    return _cloud(rng, t, rng.integers(0, C, n), V, edge, None), want


def capacity_cloud(n_inside, n_noise, seed, V=21, edge=21.0, C=5):
    """Two frames 200 Angstrom apart.  The first holds exactly n_inside encodable atoms and, interleaved with them in atom order,
    n_noise atoms that must not count: outside the cube, or inside it with channel -1 or C.  The second holds 10 atoms."""
    rng = np.random.default_rng(seed)
    ca0 = origin(rng)
    ca1 = ca0 + 200.0 * np.array([0.0, 1.0, 0.0])
    full = interior_cloud(V, edge, C, n_inside, seed + 1, ca=ca0)
    kind = rng.integers(0, 3, n_noise)
    t = np.where((kind == 0)[:, None], outside_targets(rng, n_noise, V, edge), _in_voxels(rng, rng.integers(0, V, (n_noise, 3)), V, edge))
    noise = Cloud(place(t, full.frt[0]), np.where(kind == 0, rng.integers(0, C, n_noise), np.where(kind == 1, -1, C)).astype(np.int32),
                  sigmas(rng, n_noise, voxel_edge(V, edge)), full.frt[:0])
    few = interior_cloud(V, edge, C, 10, seed + 2, ca=ca1)
    both = merge(full, noise, few)
    order = np.concatenate([rng.permutation(n_inside + n_noise), n_inside + n_noise + np.arange(10)])     # interleave; the few come last
    return subset(both, order)


def many_frames(n_frames, V, edge, C, n_atoms, seed):
    """a ball of atoms of about the cube's size and n_frames frames whose origins are atoms of it, each with its own rotation"""
    rng = np.random.default_rng(seed)
    centre = origin(rng)
    v = rng.standard_normal((n_atoms, 3))
    xyz = (centre + v / np.linalg.norm(v, axis=1, keepdims=True) * (edge * rng.random((n_atoms, 1)) ** (1.0 / 3.0))).astype(np.float32)
    frt = np.stack([frame_row(rng, xyz[i]) for i in rng.integers(0, n_atoms, n_frames)])
    return Cloud(xyz, rng.integers(-1, C + 1, n_atoms).astype(np.int32), sigmas(rng, n_atoms, voxel_edge(V, edge)), frt)


NONFINITE = (np.nan, np.inf, 1e20, -3e9)


def nonfinite_cloud(seed, V=21, edge=21.0, C=5, n=240):
    """(cloud, normal atoms bool [n], NaN frames bool [5]).  A uniform cloud around three nearby frames in which four atoms had
    one coordinate replaced (NaN, +inf, 1e20, -3e9; one atom each, a different axis in turn), followed by a copy of frame 0 with a NaN
    rotation entry and a copy of frame 1 with a NaN origin component."""
    cloud = three_frames(uniform_cloud, V, edge, C, n // 3, seed)
    xyz, frt = cloud.xyz.copy(), np.concatenate([cloud.frt, cloud.frt[:2]])
    normal = np.ones(len(xyz), bool)
    for j, bad in enumerate(NONFINITE):
        i = 7 + 31 * j
        xyz[i, j % 3] = bad
        normal[i] = False
    frt[3, 4] = np.nan
    frt[4, 10] = np.nan
    ch = cloud.ch.copy()
    ch[~normal] = np.arange(4) % C                                     # encodable channels: only the coordinate keeps them out
    return Cloud(xyz, ch, cloud.sg, frt), normal, np.array([False, False, False, True, True])


# ---- restatements of spec items 3-5 on boolean frames ------------------------------------------------------------------------

def _fma(x, y, z):
    """float32 x * y + z with one rounding.  The product of two float32 is exact in float64; the sum is rounded to float64 and then
    to float32, which differs from a true FMA only where the float64 sum lands on a float32 tie — too rare to matter for a
    restatement that is wrong on purpose."""
    return (x.astype(np.float64) * y.astype(np.float64) + z.astype(np.float64)).astype(np.float32)


def boolean_frames(cloud, V, edge, C, index="spec"):
    """uint8 [n_frames, V, V, V, C], vectorised.  index = "spec": items 3-5 as written — local = (R0 d0 + R1 d1) + R2 d2 with every
    product and sum rounded to float32, index = floor(local / a + 0.5).  "fma": the sums contracted as a compiler would without the
    kernel's `fp contract(off)`: fma(R2, d2, fma(R1, d1, R0 d0)).  "reciprocal": local * (1 / a) in place of local / a."""
    f32 = np.float32
    xyz, chn, frt = np.asarray(cloud.xyz, f32), np.asarray(cloud.ch), np.asarray(cloud.frt, f32)
    a, centre = f32(edge) / f32(V), V // 2
    out = np.zeros((frt.shape[0], V, V, V, C), np.uint8)
    for r in range(frt.shape[0]):
        R, ca = frt[r, :9].reshape(3, 3), frt[r, 9:]
        with np.errstate(invalid="ignore", over="ignore"):
            d = xyz - ca[None, :]
            if index == "fma":
                loc = np.stack([_fma(R[i, 2], d[:, 2], _fma(R[i, 1], d[:, 1], R[i, 0] * d[:, 0])) for i in range(3)], axis=1)
            else:
                loc = np.stack([(R[i, 0] * d[:, 0] + R[i, 1] * d[:, 1]) + R[i, 2] * d[:, 2] for i in range(3)], axis=1).astype(f32)
            q = np.floor(loc * (f32(1.0) / a) + f32(0.5)) if index == "reciprocal" else np.floor(loc / a + f32(0.5))
        ok = np.all((q >= f32(-centre)) & (q <= f32(V - 1 - centre)), axis=1) & (chn >= 0) & (chn < C)
        i = q[ok].astype(np.int64) + centre
        out[r, i[:, 0], i[:, 1], i[:, 2], chn[ok]] = 1
    return out


# ---- the clouds the GPU sweep runs, by name, so that the host tests can hold each of them to the kernel's limits ---------------

def sweep_boolean(V, edge, C):
    return Case(three_frames(face_cloud, V, edge, C, 600, 1000 + 7 * V + C), V, edge, C)


def sweep_gaussian(V, edge, C):
    return Case(three_frames(uniform_cloud, V, edge, C, 200, 2000 + 7 * V + C), V, edge, C)


def chunking(gaussian):
    cloud, want = chunked_cloud(21, 21.0, 5, 5000, 0.06 if gaussian else 0.45, 31)
    return Case(cloud, 21, 21.0, 5), want


def borders(V):
    edge = {5: 7.3, 21: 20.0}[V]
    return Case(three_frames(border_cloud, V, edge, 5, 150, 40 + V), V, edge, 5)


def interiors(V):
    edge = {5: 7.3, 21: 20.0}[V]
    # one frame: no atom of another frame near its border.  27 inner voxels at V = 5: 60 atoms keep a cell's overlap near 10 per channel
    return Case(interior_cloud(V, edge, 5, 60 if V == 5 else 300, 50 + V), V, edge, 5)


def stacked(C, channel):
    return Case(stacked_cloud(9, 12.5, C, 120, 60 + C, channel=channel), 9, 12.5, C)


def one_launch_cases():
    """name -> Case for every cloud the GPU sweep voxelises in one launch and expects to succeed"""
    cases = {}
    for V, edge, C in SWEEP:
        cases[f"sweep-bool-{V}-{edge}-{C}"] = sweep_boolean(V, edge, C)
        cases[f"sweep-gauss-{V}-{edge}-{C}"] = sweep_gaussian(V, edge, C)
    for gaussian in (False, True):
        cases[f"chunking-{'gauss' if gaussian else 'bool'}"] = chunking(gaussian)[0]
    for V in (5, 21):
        cases[f"borders-{V}"] = borders(V)
        cases[f"interiors-{V}"] = interiors(V)
    cases["stacked-1"] = stacked(1, 0)
    cases["stacked-7"] = stacked(7, 6)
    cases["capacity-2048"] = Case(capacity_cloud(MAX_LIST, 1500, 70), 21, 21.0, 5)
    cases["batch-300"] = Case(many_frames(300, 5, 7.3, 4, 400, 80), 5, 7.3, 4)
    cases["batch-3"] = Case(many_frames(3, 21, 21.0, 5, 500, 81), 21, 21.0, 5)
    cases["nonfinite"] = Case(nonfinite_cloud(90)[0], 21, 21.0, 5)
    return cases


GAUSSIAN_CASES = ("sweep-gauss", "chunking-gauss", "borders", "interiors", "stacked", "batch", "nonfinite")


# ---- what the two GPU test files share ------------------------------------------------------------------------------------------

RTOL, ATOL = 5e-6, 1e-9               # Gaussian frames against the oracle: expf against NumPy's float32 exp


def same(got, want, gaussian, label):
    """boolean frames bit-exact; Gaussian frames the same non-zero voxels and values within RTOL, ATOL"""
    assert got.dtype == want.dtype and got.shape == want.shape
    if not gaussian:
        print(f"{label}: {int(want.sum())} cells set, {int(np.count_nonzero(got != want))} differ")
        assert np.array_equal(got, want)                                      # bit-exact
        return
    g, w = got.astype(np.float64), want.astype(np.float64)
    worst = float(np.max(np.abs(g - w) / (ATOL + RTOL * np.abs(w)))) if w.size else 0.0
    print(f"{label}: {int(np.count_nonzero(want))} non-zero, support differs in {int(np.count_nonzero((got != 0) != (want != 0)))}, "
          f"worst |got - want| / (atol + rtol |want|) = {worst:.3f}")
    assert not np.isnan(got).any()
    assert np.array_equal(got != 0, want != 0)                                # the same voxels are touched
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)


def decoy(cloud, C):
    """the same coordinates with the encodable channels rotated by one, and no frame"""
    ch = np.where((cloud.ch >= 0) & (cloud.ch < C), (cloud.ch + 1) % C, cloud.ch).astype(np.int32)
    return Cloud(cloud.xyz, ch, cloud.sg, cloud.frt[:0])


def mixed_clouds():
    """(18 clouds, (V, edge, C)): nine structures of the (21, 21.0, 5) geometry, each followed by its decoy"""
    V, edge, C = 21, 21.0, 5
    cases = one_launch_cases()
    row = frame_row(np.random.default_rng(5))
    real = [cases["batch-3"].cloud, Cloud(np.zeros((0, 3), np.float32), np.zeros(0, np.int32), np.zeros(0, np.float32), row[None, :]),
            cases["chunking-gauss"].cloud]
    real += [interior_cloud(V, edge, C, 1, 701)] + [uniform_cloud(V, edge, C, n, 700 + n) for n in (255, 256, 257)]
    real += [cases["nonfinite"].cloud, Cloud(*uniform_cloud(V, edge, C, 300, 990)[:3], np.zeros((0, 12), np.float32))]
    return [c for r in real for c in (r, decoy(r, C))], (V, edge, C)


def weight_inputs():
    """(case, weights from {-1, 1, 2.5}, signs +-1, channels that put the positive atoms in 0 and the negative ones in 1): what the
    weights test of tests/test_gpu_voxelise_batch.py feeds the kernel"""
    case = sweep_gaussian(9, 12.5, 8)
    cloud = case.cloud
    rng = np.random.default_rng(17)
    wgt = rng.choice(np.array([-1.0, 1.0, 2.5], np.float32), len(cloud.xyz))
    keep = (cloud.ch >= 0) & (cloud.ch < case.C)
    sign = np.where(rng.random(len(cloud.xyz)) < 0.5, -1.0, 1.0).astype(np.float32)
    two = np.where(keep, np.where(sign > 0, 0, 1), -1).astype(np.int32)
    return case, wgt, sign, two


# ---- the bytes of the commit before the two voxeliser kernels became one (tests/golden/voxelise_digests.json) -------------------

UBQ_DIGEST = "1ubq/five"              # the 76 five-channel Gaussian frames of tests/golden/1ubq.pdb1.gz


def digest_cases():
    """[(id, cloud, V, edge, C, gaussian)]: every synthetic th_voxelise call whose bytes tests/golden/make_voxelise_digests.py records"""
    calls = []
    for V, edge, C in SWEEP:
        for which, case in (("bool-cloud", sweep_boolean(V, edge, C)), ("gauss-cloud", sweep_gaussian(V, edge, C))):
            calls += [(f"sweep/{V}-{edge}-{C}/{which}/{mode(g)}", case.cloud, V, edge, C, g) for g in (False, True)]
    clouds, (V, edge, C) = mixed_clouds()
    calls += [(f"mixed/{s}/{mode(g)}", c, V, edge, C, g) for s, c in enumerate(clouds) for g in (False, True)]
    case = one_launch_cases()["batch-300"]
    calls += [(f"batch-300/{mode(g)}", case.cloud, case.V, case.edge, case.C, g) for g in (False, True)]
    case, _wgt, _sign, two = weight_inputs()
    calls.append(("weights/unit", case.cloud, case.V, case.edge, case.C, True))
    calls.append(("weights/two-channel", Cloud(case.cloud.xyz, two, case.cloud.sg, case.cloud.frt), case.V, case.edge, 2, True))
    return calls


def mode(gaussian):
    return "gaussian" if gaussian else "boolean"


def digest(frames):
    a = np.ascontiguousarray(frames)
    return dict(shape=list(a.shape), dtype=str(a.dtype), sha256=hashlib.sha256(a.tobytes()).hexdigest())


_RECORDED = {}


def assert_parent_bytes(frames, case_id):
    """shape, dtype and SHA-256 of ``frames`` are those recorded under ``case_id`` at the parent commit"""
    if not _RECORDED:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "voxelise_digests.json")) as f:
            _RECORDED.update(json.load(f)["cases"])
    assert digest(frames) == _RECORDED[case_id], case_id
