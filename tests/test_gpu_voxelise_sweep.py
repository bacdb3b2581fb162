"""th_voxelise (csrc/voxelise.hip: the one-structure call of the kernel th_voxelise_batch runs) against oracle/voxel_oracle.py away from the one geometry of tests/test_voxeliser.py: voxel edges
that are not 1, atoms on voxel faces, 1..8 channels, atoms spread over twenty compaction chunks, the atom list at its limit and one
past it, atoms at the cube's border, stacked atoms, hundreds of frames in a launch, non-finite input, boolean frames kept on the
device.  The clouds come from tests/voxel_cases.py; tests/test_voxel_cases_host.py shows on the CPU what they can tell apart.

Tolerances are those of tests/test_voxeliser.py: boolean frames bit-exact; Gaussian frames with the same non-zero voxels and values
within rtol 5e-6, atol 1e-9 (expf against NumPy's float32 exp): voxel_cases.same."""
import numpy as np
import pytest

import voxel_cases as vc
from oracle import voxel_oracle
from timed_hip import _lib, voxeliser

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return vc.one_launch_cases()


_ORACLE = {}


def _want(cases, name, gaussian):
    """the oracle's frames of a named case, computed once per module run and never written to"""
    key = (name, gaussian)
    if key not in _ORACLE:
        case = cases[name]
        _ORACLE[key] = voxel_oracle.voxelise(*case.cloud, case.V, case.edge, case.C, gaussian)
        _ORACLE[key].setflags(write=False)
    return _ORACLE[key]


def _run(case, gaussian, gpu, cloud=None, **kw):
    return voxeliser.voxelise(*(case.cloud if cloud is None else cloud), case.V, case.edge, case.C, gaussian, device=gpu, **kw)


# ---- a. geometry sweep ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gaussian", [False, True])
@pytest.mark.parametrize("V,edge,C", vc.SWEEP)
def test_geometry_sweep(gpu, cases, V, edge, C, gaussian):
    """atoms on voxel faces (boolean) and anywhere (Gaussian), three frames each with its own rotation and origin, voxel edges
    20/21, 1, 12.5/9, 7.3/5, 2/3 and 4: a contracted or approximately divided index fails the boolean cases"""
    name = f"sweep-{'gauss' if gaussian else 'bool'}-{V}-{edge}-{C}"
    want = _want(cases, name, gaussian)
    assert want.shape == (3, V, V, V, C) and want.any()
    vc.same(_run(cases[name], gaussian, gpu), want, gaussian, name)


# ---- b. chunking ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gaussian", [False, True])
def test_atoms_inside_scattered_over_twenty_chunks(gpu, cases, gaussian):
    """5000 atoms: chunks with no atom inside, with whole waves inside, with a sprinkle, and a partial last chunk"""
    name = f"chunking-{'gauss' if gaussian else 'bool'}"
    vc.same(_run(cases[name], gaussian, gpu), _want(cases, name, gaussian), gaussian, name)


# ---- c. capacity ---------------------------------------------------------------------------------------------------------------

def test_atom_list_exactly_full(gpu, cases):
    """2048 encodable atoms inside one frame, interleaved with 1500 that are outside or of channel -1 or C and must not count"""
    vc.same(_run(cases["capacity-2048"], False, gpu), _want(cases, "capacity-2048", False), False, "capacity-2048")


def test_atom_list_one_too_many(gpu, lib):
    """2049 in the first frame, 10 in the second: the whole call fails with TH_EUNSUP and names the count"""
    case = vc.Case(vc.capacity_cloud(vc.MAX_LIST + 1, 0, 71), 21, 21.0, 5)
    with pytest.raises(_lib.TimedHipError) as err:
        _run(case, False, gpu)
    print(err.value)
    assert err.value.code == -4 and "2049 encodable atoms" in str(err.value)
    assert b"2049" in lib.th_last_error()
    # the second frame alone is fine, and the library is usable after the refusal
    alone = vc.Cloud(*case.cloud[:3], case.cloud.frt[1:])
    got = _run(case, False, gpu, cloud=alone)
    assert np.array_equal(got, voxel_oracle.voxelise(*alone, 21, 21.0, 5, False)) and got.sum() == 10


# ---- d. borders ----------------------------------------------------------------------------------------------------------------

def _encodable(case):
    ch_ok = (case.cloud.ch >= 0) & (case.cloud.ch < case.C)
    return [int((voxel_oracle.locate(case.cloud.xyz, row, case.V, case.edge)[2] & ch_ok).sum()) for row in case.cloud.frt]


@pytest.mark.parametrize("V", [5, 21])
def test_weight_beyond_the_border_is_lost(gpu, cases, V):
    name = f"borders-{V}"
    got, want = _run(cases[name], True, gpu), _want(cases, name, True)
    vc.same(got, want, True, name)
    for r, n in enumerate(_encodable(cases[name])):
        lost_got, lost_want = n - got[r].sum(dtype=np.float64), n - want[r].sum(dtype=np.float64)
        print(f"{name} frame {r}: {n} atoms inside, mass lost {lost_got:.6f} (oracle {lost_want:.6f})")
        assert lost_want > 0.05 * n                                   # the case does lose mass
        assert abs(lost_got - lost_want) <= 1e-5 * n


@pytest.mark.parametrize("V", [5, 21])
def test_interior_atoms_keep_unit_mass(gpu, cases, V):
    """27 correctly rounded quotients of a 26-addition float32 total, accumulated in float32 over ~10-20 overlapping atoms: ~3e-6 per
    atom; 1e-5 allowed"""
    name = f"interiors-{V}"
    case = cases[name]
    got = _run(case, True, gpu)
    vc.same(got, _want(cases, name, True), True, name)
    count = np.bincount(case.cloud.ch, minlength=case.C)
    mass = got[0].reshape(-1, case.C).sum(axis=0, dtype=np.float64)
    print(f"{name}: atoms per channel {count.tolist()}, |mass - count| / count {(np.abs(mass - count) / count).tolist()}")
    assert count.min() > 0 and np.all(np.abs(mass - count) <= 1e-5 * count)


# ---- e. stacking and channels --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C,channel", [(1, 0), (7, 6)])
def test_stacked_atoms(gpu, cases, C, channel):
    """120 atoms of one channel in four voxels: a boolean cell stays 1, a Gaussian cell holds the sum"""
    name = f"stacked-{C}"
    b = _run(cases[name], False, gpu)
    vc.same(b, _want(cases, name, False), False, name)
    assert b.max() == 1 and 1 <= b.sum() <= 4 and b[..., channel].sum() == b.sum()
    g = _run(cases[name], True, gpu)
    vc.same(g, _want(cases, name, True), True, name)
    assert g.max() > 2.0 and g[..., channel].sum(dtype=np.float64) == g.sum(dtype=np.float64)


@pytest.mark.parametrize("C", [1, 7])
def test_channels_out_of_range_leave_no_trace_and_bytes_are_stored_one_by_one(gpu, C):
    """uint8 frames of 1 and 7 channels (odd strides: every channel byte is a store of its own); atoms of channel -1 and C vanish"""
    cloud = vc.uniform_cloud(9, 12.5, C, 500, 600 + C)
    case = vc.Case(cloud, 9, 12.5, C)
    assert {-1, C} <= set(cloud.ch.tolist())
    keep = (cloud.ch >= 0) & (cloud.ch < C)
    for gaussian in (False, True):
        got = _run(case, gaussian, gpu)
        assert np.array_equal(got, _run(case, gaussian, gpu, cloud=vc.subset(cloud, keep)))
        if not gaussian:
            want = voxel_oracle.voxelise(*cloud, 9, 12.5, C, False)
            vc.same(got, want, False, f"channels-{C}")
            assert all(want[..., c].any() for c in range(C))


# ---- f. batch independence -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gaussian", [False, True])
@pytest.mark.parametrize("name", ["batch-300", "batch-3"])
def test_frames_do_not_depend_on_their_launch(gpu, cases, name, gaussian):
    case = cases[name]
    full = _run(case, gaussian, gpu)
    assert full.any(axis=(1, 2, 3, 4)).all()
    assert full.tobytes() == _run(case, gaussian, gpu).tobytes()              # the same launch twice: the same bytes
    for r in range(len(case.cloud.frt)):
        single = _run(case, gaussian, gpu, cloud=vc.Cloud(*case.cloud[:3], case.cloud.frt[r:r + 1]))
        assert np.array_equal(single[0], full[r]), r
    if name == "batch-3":
        vc.same(full, _want(cases, name, gaussian), gaussian, name)


# ---- g. non-finite input -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gaussian", [False, True])
def test_non_finite_atoms_and_frames_are_not_encoded(gpu, gaussian):
    """Spec item 4: an atom with a NaN, infinite or absurdly large coordinate is not encoded, and a frame whose row holds a NaN is
    all zeros.  (Before the inside test moved in front of the integer conversion, v_cvt_i32_f32 turned NaN into index 0: such an
    atom landed in the centre voxel, and a NaN frame collected every atom of the structure there.)"""
    cloud, normal, nan_frames = vc.nonfinite_cloud(90)
    case = vc.Case(cloud, 21, 21.0, 5)
    got = _run(case, gaussian, gpu)
    want = voxel_oracle.voxelise(*vc.subset(cloud, normal), 21, 21.0, 5, gaussian)     # the finite atoms alone
    print(f"non-finite, gaussian={gaussian}: NaNs in the output {int(np.isnan(got).sum())}; non-zero cells in the two NaN frames "
          f"{[int(np.count_nonzero(f)) for f in got[nan_frames]]}; cells that differ from the finite atoms' frames "
          f"{[int(np.count_nonzero(g != w)) for g, w in zip(got[~nan_frames], want[~nan_frames])]}")
    assert not np.isnan(got).any()
    assert not got[nan_frames].any()
    assert want[~nan_frames].any(axis=(1, 2, 3, 4)).all()
    vc.same(got[~nan_frames], want[~nan_frames], gaussian, "non-finite")


# ---- h. boolean frames on the device -------------------------------------------------------------------------------------------

def test_boolean_frames_stay_on_the_device_for_the_cnn(gpu, cases):
    from timed_hip import engine, synth
    case = cases["batch-3"]
    n, V, C = len(case.cloud.frt), case.V, case.C
    host = _run(case, False, gpu)
    vc.same(host, _want(cases, "batch-3", False), False, "device-uint8")
    d_frames = engine.DeviceBuffer(host.nbytes + 64, gpu)
    d_frames.upload(np.full(host.nbytes + 64, 0xAB, np.uint8))                 # every byte of the frames must be written, none beyond
    assert _run(case, False, gpu, d_out=d_frames.ptr) is None
    assert np.array_equal(d_frames.download(host.shape, np.uint8), host)
    assert np.all(d_frames.download(64, np.uint8, offset=host.nbytes) == 0xAB)
    cfg, weights = synth.timed_synth(20, widths=(8, 16), side=V, in_channels=C, seed=3)
    model = engine.HipFrameModel.from_keras(cfg, weights, device=gpu)
    d_probs = engine.DeviceBuffer(n * 20 * 4, gpu)
    model.predict_device(d_frames.ptr, n, d_probs.ptr, dtype=_lib.TH_U8)
    on_device = d_probs.download((n, 20), np.float32)
    assert np.array_equal(model.predict(host), on_device)
    np.testing.assert_allclose(on_device.sum(1), 1.0, atol=1e-5)
