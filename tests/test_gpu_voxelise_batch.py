"""th_voxelise_batch (csrc/voxelise.hip) on the GPU: many structures in one launch against the per-structure oracle
(oracle/voxel_oracle.py); byte for byte against one th_voxelise call per structure (the same kernel through the one-structure
wrapper: stack offsets, a zeroed frame_structure) and, both of them, against the digests of the frames th_voxelise gave at 51dee49,
when it still had a kernel of its own (tests/golden/voxelise_digests.json); frames that do not depend on their batch;
the atom list at its limit and one past it in the middle of a batch; weights against the restatement
(tests/voxel_weight_restatement.py) and against a difference of two unit-weight channels; frames written into the middle of a device
buffer and read there by the CNN; the charge channel of 1ubq.  Clouds from tests/voxel_cases.py.

Tolerances are those of tests/test_gpu_voxelise_sweep.py: boolean frames bit-exact; Gaussian frames the same non-zero voxels, rtol
5e-6, atol 1e-9.  Weighted frames: |got - want| <= 1e-9 + 5e-6 * (frames of |weight|) — where contributions of both signs meet, a
bound relative to the difference would mean nothing."""
import os

import numpy as np
import pytest

import voxel_cases as vc
import voxel_weight_restatement as vw
from oracle import voxel_oracle
from timed_hip import _lib, voxeliser

pytestmark = pytest.mark.gpu

RTOL, ATOL = vc.RTOL, vc.ATOL
UBQ = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "1ubq.pdb1.gz")


def _flatten(clouds, order_seed=None):
    """the arguments of one batch call for a list of clouds (one structure each); frames interleaved when a seed is given.
    Returns (kwargs, [(structure, frame row of that structure)] in batch order)."""
    sizes = [len(c.xyz) for c in clouds]
    frames = [(s, k) for s, c in enumerate(clouds) for k in range(len(c.frt))]
    if order_seed is not None:
        frames = [frames[i] for i in np.random.default_rng(order_seed).permutation(len(frames))]
    kw = dict(atoms_xyz=np.concatenate([c.xyz for c in clouds]), atom_channel=np.concatenate([c.ch for c in clouds]),
              atom_sigma=np.concatenate([c.sg for c in clouds]), atom_weight=None,
              atom_offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64),
              frames_rt=np.array([clouds[s].frt[k] for s, k in frames], np.float32).reshape(-1, 12),
              frame_structure=np.array([s for s, _ in frames], np.int32))
    return kw, frames


def _per_structure(got, frames, n_structures):
    """the frames of a batch regrouped: one array per structure, in that structure's own frame order"""
    where = {sk: r for r, sk in enumerate(frames)}
    return [got[[where[(s, k)] for k in range(sum(1 for t, _ in frames if t == s))]] for s in range(n_structures)]


def _within_mass(got, want, mass, label):
    """|got - want| <= 1e-9 + 5e-6 * mass, mass being the frames of |weight|"""
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    bound = ATOL + RTOL * mass.astype(np.float64)
    print(f"{label}: {int(np.count_nonzero(mass))} voxels touched, worst |got - want| / bound = {float((err / bound).max()):.3f}")
    assert not np.isnan(got).any() and np.all(err <= bound)


# ---- a. one batch of everything ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mixed():
    """structures of the (21, 21.0, 5) geometry, each followed by its decoy; the oracle's frames per structure, computed once"""
    clouds, (V, edge, C) = vc.mixed_clouds()
    real = clouds[::2]
    assert [len(c.xyz) for c in real] == [500, 0, 5000, 1, 255, 256, 257, 240, 300] and [len(c.frt) for c in real] == [3, 1, 1, 1, 1, 1, 1, 5, 0]
    starts = np.concatenate([[0], np.cumsum([len(c.xyz) for c in clouds])])[:-1]
    assert sum(1 for c, o in zip(clouds, starts) if len(c.frt) and o % vc.CHUNK) >= 6         # ranges that start off a chunk boundary
    want = {g: [voxel_oracle.voxelise(*c, V, edge, C, g) for c in clouds] for g in (False, True)}
    for frames in want.values():
        for f in frames:
            f.setflags(write=False)
    return clouds, want, (V, edge, C)


@pytest.mark.parametrize("gaussian", [False, True])
def test_one_batch_of_many_structures(gpu, mixed, gaussian):
    clouds, want, (V, edge, C) = mixed
    kw, frames = _flatten(clouds, order_seed=11)
    assert [s for s, _ in frames] != sorted(s for s, _ in frames)                         # interleaved, not grouped by structure
    got = voxeliser.voxelise_batch(**kw, voxels_per_side=V, frame_edge_length=edge, n_channels=C, gaussian=gaussian, device=gpu)
    expect = np.stack([want[gaussian][s][k] for s, k in frames])
    vc.same(got, expect, gaussian, f"mixed batch, gaussian={gaussian}")
    assert expect.any(axis=(1, 2, 3, 4)).sum() == 11                                      # all but the empty structure's and the two NaN frames
    # the bytes of one th_voxelise call per structure, and of both the bytes of the parent's th_voxelise
    single = [voxeliser.voxelise(*c, V, edge, C, gaussian, device=gpu) for c in clouds]
    assert got.tobytes() == np.stack([single[s][k] for s, k in frames]).tobytes()
    for s, (mine, alone) in enumerate(zip(_per_structure(got, frames, len(clouds)), single)):
        vc.assert_parent_bytes(mine, f"mixed/{s}/{vc.mode(gaussian)}")
        vc.assert_parent_bytes(alone, f"mixed/{s}/{vc.mode(gaussian)}")
    # the same batch again, and every frame in a batch of its own that holds nothing but its structure
    again = voxeliser.voxelise_batch(**kw, voxels_per_side=V, frame_edge_length=edge, n_channels=C, gaussian=gaussian, device=gpu)
    assert again.tobytes() == got.tobytes()
    for r, (s, k) in enumerate(frames):
        c = clouds[s]
        alone = voxeliser.voxelise_batch(c.xyz, c.ch, c.sg, None, [0, len(c.xyz)], c.frt[k:k + 1], [0], V, edge, C, gaussian, device=gpu)
        assert alone[0].tobytes() == got[r].tobytes(), (r, s, k)


@pytest.mark.parametrize("gaussian", [False, True])
def test_every_sweep_geometry_gives_the_bytes_of_th_voxelise(gpu, gaussian):
    """voxel grids of 1, 3, 5, 9 and 21 planes, 1 to 8 channels, two structures per batch (the face clouds and the uniform ones):
    the planes the gather walks are the cube's first and last ones as well"""
    for V, edge, C in vc.SWEEP:
        clouds = [vc.sweep_boolean(V, edge, C).cloud, vc.sweep_gaussian(V, edge, C).cloud]
        kw, frames = _flatten(clouds, order_seed=V + C)
        got = voxeliser.voxelise_batch(**kw, voxels_per_side=V, frame_edge_length=edge, n_channels=C, gaussian=gaussian, device=gpu)
        single = [voxeliser.voxelise(*c, V, edge, C, gaussian, device=gpu) for c in clouds]
        assert got.any() and got.tobytes() == np.stack([single[s][k] for s, k in frames]).tobytes(), (V, edge, C)
        for which, mine, alone in zip(("bool-cloud", "gauss-cloud"), _per_structure(got, frames, 2), single):
            vc.assert_parent_bytes(mine, f"sweep/{V}-{edge}-{C}/{which}/{vc.mode(gaussian)}")
            vc.assert_parent_bytes(alone, f"sweep/{V}-{edge}-{C}/{which}/{vc.mode(gaussian)}")


# ---- b. many frames --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gaussian", [False, True])
def test_three_hundred_frames_twice(gpu, gaussian):
    case = vc.one_launch_cases()["batch-300"]
    kw, frames = _flatten([case.cloud, case.cloud])
    got = voxeliser.voxelise_batch(**kw, voxels_per_side=case.V, frame_edge_length=case.edge, n_channels=case.C, gaussian=gaussian, device=gpu)
    single = voxeliser.voxelise(*case.cloud, case.V, case.edge, case.C, gaussian, device=gpu)
    assert got.shape == (600, 5, 5, 5, 4) and single.any(axis=(1, 2, 3, 4)).all()
    assert got[:300].tobytes() == single.tobytes() and got[300:].tobytes() == single.tobytes()
    for frames_of_one in (got[:300], got[300:], single):
        vc.assert_parent_bytes(frames_of_one, f"batch-300/{vc.mode(gaussian)}")


# ---- c. capacity -----------------------------------------------------------------------------------------------------------------

def test_atom_list_full_and_one_too_many_in_the_middle_of_a_batch(gpu, lib):
    V, edge, C = 21, 21.0, 5
    side = [vc.uniform_cloud(V, edge, C, 200, 801), vc.uniform_cloud(V, edge, C, 130, 802)]
    full = vc.capacity_cloud(vc.MAX_LIST, 1500, 70)
    clouds = [side[0], full, side[1]]
    kw, frames = _flatten(clouds)
    got = voxeliser.voxelise_batch(**kw, voxels_per_side=V, frame_edge_length=edge, n_channels=C, gaussian=False, device=gpu)
    want = np.concatenate([voxel_oracle.voxelise(*c, V, edge, C, False) for c in clouds])
    vc.same(got, want, False, "capacity-2048 between two structures")
    assert int(want[1].sum()) > 1500
    over, _ = _flatten([side[0], vc.capacity_cloud(vc.MAX_LIST + 1, 0, 71), side[1]])
    with pytest.raises(_lib.TimedHipError) as err:
        voxeliser.voxelise_batch(**over, voxels_per_side=V, frame_edge_length=edge, n_channels=C, gaussian=False, device=gpu)
    print(err.value)
    assert err.value.code == -4 and "2049" in str(err.value) and b"2049" in lib.th_last_error() and "th_voxelise_batch" in str(err.value)
    after = voxeliser.voxelise_batch(**kw, voxels_per_side=V, frame_edge_length=edge, n_channels=C, gaussian=False, device=gpu)
    assert after.tobytes() == got.tobytes()


@pytest.mark.parametrize("V,edge", [(5, 7.3), (21, 21.0)])
def test_th_voxelise_reports_the_largest_of_two_overflowing_frames(gpu, lib, V, edge):
    """one structure, two frames that both overflow (2049 and 2100 encodable atoms): the count in the message is the larger one
    whichever workgroup wrote last, call after call, and the next valid call is unharmed"""
    C = 5
    a, b = vc.capacity_cloud(vc.MAX_LIST + 1, 0, 171, V, edge, C), vc.capacity_cloud(2100, 0, 172, V, edge, C)
    both = vc.merge(a, b)                                                                 # frames: a's full one, a's few, b's full one, b's few
    ch_ok = (both.ch >= 0) & (both.ch < C)
    inside = [int((voxel_oracle.locate(both.xyz, row, V, edge)[2] & ch_ok).sum()) for row in both.frt]
    assert inside == [2049, 10, 2100, 10]
    for _ in range(3):
        with pytest.raises(_lib.TimedHipError) as err:
            voxeliser.voxelise(both.xyz, both.ch, both.sg, both.frt[[0, 2]], V, edge, C, False, device=gpu)
        assert err.value.code == -4 and "2100 encodable atoms" in str(err.value) and b"2100" in lib.th_last_error()
        assert "th_voxelise:" in str(err.value) and "th_voxelise_batch" not in str(err.value)
    few = voxeliser.voxelise(both.xyz, both.ch, both.sg, both.frt[[1, 3]], V, edge, C, False, device=gpu)
    want = voxel_oracle.voxelise(both.xyz, both.ch, both.sg, both.frt[[1, 3]], V, edge, C, False)
    assert want.any(axis=(1, 2, 3, 4)).all() and few.tobytes() == want.tobytes()


# ---- d. weights ------------------------------------------------------------------------------------------------------------------

def test_weights_against_the_restatement_and_against_two_channels(gpu):
    case, wgt, sign, two = vc.weight_inputs()
    cloud, V, edge, C = case.cloud, case.V, case.edge, case.C
    off, fst = [0, len(cloud.xyz)], np.zeros(len(cloud.frt), np.int32)
    got = voxeliser.voxelise_batch(cloud.xyz, cloud.ch, cloud.sg, wgt, off, cloud.frt, fst, V, edge, C, True, device=gpu)
    want, mass = vw.voxelise_weighted(cloud.xyz, cloud.ch, cloud.sg, wgt, cloud.frt, V, edge, C)
    _within_mass(got, want, mass, "weights {-1, 1, 2.5}")
    unit = voxeliser.voxelise(*cloud, V, edge, C, True, device=gpu)
    print(f"support: weighted {int(np.count_nonzero(got))}, restated {int(np.count_nonzero(want))}, unit weights {int(np.count_nonzero(unit))}")
    assert np.array_equal(got != 0, want != 0) and np.array_equal(got != 0, unit != 0)
    assert (got < 0).any() and (got > 1).any()
    # all ones: the bytes of th_voxelise
    ones = voxeliser.voxelise_batch(cloud.xyz, cloud.ch, cloud.sg, np.ones(len(cloud.xyz), np.float32), off, cloud.frt, fst, V, edge, C, True, device=gpu)
    assert ones.tobytes() == unit.tobytes()
    vc.assert_parent_bytes(unit, "weights/unit")
    vc.assert_parent_bytes(ones, "weights/unit")
    # without the restatement: positive atoms in channel 0 and negative ones in channel 1 at unit weight, against all of them in
    # channel 0 with weights +-1
    keep = (cloud.ch >= 0) & (cloud.ch < C)
    old = voxeliser.voxelise(cloud.xyz, two, cloud.sg, cloud.frt, V, edge, 2, True, device=gpu)
    vc.assert_parent_bytes(old, "weights/two-channel")
    new = voxeliser.voxelise_batch(cloud.xyz, np.where(keep, 0, -1).astype(np.int32), cloud.sg, sign, off, cloud.frt, fst, V, edge, 1, True, device=gpu)
    assert old[..., 0].any() and old[..., 1].any() and ((old[..., 0] != 0) & (old[..., 1] != 0)).any()
    _within_mass(new[..., 0], old[..., 0].astype(np.float64) - old[..., 1].astype(np.float64), old[..., 0].astype(np.float64) + old[..., 1], "+-1 against two channels")


# ---- e. device output ------------------------------------------------------------------------------------------------------------

def test_frames_written_into_the_middle_of_a_device_buffer_feed_the_cnn(gpu):
    from timed_hip import engine, synth
    V, edge, C = 21, 21.0, 5
    clouds = [vc.one_launch_cases()["batch-3"].cloud, vc.uniform_cloud(V, edge, C, 257, 957)]
    kw, frames = _flatten(clouds, order_seed=3)
    n = len(frames)
    host = voxeliser.voxelise_batch(**kw, voxels_per_side=V, frame_edge_length=edge, n_channels=C, gaussian=True, device=gpu)
    assert host.any(axis=(1, 2, 3, 4)).all()
    front, back = 512, 256
    d_frames = engine.DeviceBuffer(front + host.nbytes + back, gpu)
    d_frames.upload(np.full(front + host.nbytes + back, 0xAB, np.uint8))
    timing = {}
    assert voxeliser.voxelise_batch(**kw, voxels_per_side=V, frame_edge_length=edge, n_channels=C, gaussian=True, device=gpu,
                                    d_out=d_frames.ptr + front, timing=timing) is None
    assert timing["kernel_ms"] > 0
    raw = d_frames.download(front + host.nbytes + back, np.uint8)
    assert np.all(raw[:front] == 0xAB) and np.all(raw[front + host.nbytes:] == 0xAB)
    assert raw[front:front + host.nbytes].tobytes() == host.tobytes()
    # every byte was written: the same call over a buffer filled with another pattern leaves the same bytes
    d_frames.upload(np.full(front + host.nbytes + back, 0x5C, np.uint8))
    voxeliser.voxelise_batch(**kw, voxels_per_side=V, frame_edge_length=edge, n_channels=C, gaussian=True, device=gpu, d_out=d_frames.ptr + front)
    assert d_frames.download(host.nbytes, np.uint8, offset=front).tobytes() == host.tobytes()
    cfg, weights = synth.timed_synth(20, widths=(8, 16), side=V, in_channels=C, seed=3)
    model = engine.HipFrameModel.from_keras(cfg, weights, device=gpu)
    d_probs = engine.DeviceBuffer(n * 20 * 4, gpu)
    model.predict_device(d_frames.ptr + front, n, d_probs.ptr)
    on_device = d_probs.download((n, 20), np.float32)
    assert np.array_equal(model.predict(host), on_device)
    np.testing.assert_allclose(on_device.sum(1), 1.0, atol=1e-5)


# ---- f. the charge channel of 1ubq -----------------------------------------------------------------------------------------------

def test_charge_channel_of_1ubq(gpu, tmp_path):
    from timed_hip import pdbio
    five, _, flat = voxeliser.voxelise_pdb(UBQ, device=gpu)
    assert five.shape == (76, 21, 21, 21, 5)
    vc.assert_parent_bytes(five, vc.UBQ_DIGEST)
    for value in (1, -1, 0):
        six, labels, flat6 = voxeliser.voxelise_pdb(UBQ, device=gpu, property="charge", property_map=[value] * 76)
        assert six.shape == (76, 21, 21, 21, 6) and flat6 == flat and labels.shape == (76, 20)
        assert six[..., :5].tobytes() == five.tobytes(), value
        ca = np.ascontiguousarray(six[..., 3])
        assert ca.any(axis=(1, 2, 3)).all()
        # the negation as the kernel forms it, 0 - x: an untouched voxel stays +0.0 (NumPy's unary minus would make it -0.0)
        want = ca if value == 1 else np.float32(0.0) - ca if value == -1 else np.zeros_like(ca)
        assert np.ascontiguousarray(six[..., 5]).tobytes() == want.tobytes(), value           # bit for bit
    native, labels, _ = voxeliser.voxelise_pdb(UBQ, device=gpu, property="charge")
    assert native[..., :5].tobytes() == five.tobytes()
    xyz, ch, sg, wt, frt, _ = voxeliser.prepare_structure_with_property(pdbio.read_pdb(UBQ)[0], "charge")
    q = ch == 5
    assert int(q.sum()) == 24
    want, mass = vw.voxelise_weighted(xyz[q], ch[q], sg[q], wt[q], frt, 21, 21.0, 6)
    assert not want[..., :5].any() and (want[..., 5] > 0).any() and (want[..., 5] < 0).any()
    _within_mass(native[..., 5], want[..., 5], mass[..., 5], "native charge map of 1ubq")
    assert np.array_equal(native[..., 5] != 0, mass[..., 5] != 0)
    # such frames as an .hdf5 in aposteriori's layout: six names in the atom encoder, the frames read back as they are
    from design_utils import utils as du
    from timed_hip import h5lite
    h5 = tmp_path / "charge.hdf5"
    voxeliser.write_hdf5(h5, native[:3], labels[:3], flat[:3], gaussian=True, atom_encoder=voxeliser.property_encoder("charge"))
    with h5lite.File(str(h5)) as f:
        assert list(f.attrs["atom_encoder"]) == ["C", "N", "O", "CA", "CB", "Q"] and tuple(f.attrs["frame_dims"]) == (21, 21, 21, 6)
    back, _ = du.load_batch(h5, flat[:3])
    assert np.array_equal(back.astype(np.float32), native[:3])
