"""CPU checks of tests/voxel_cases.py — that the clouds the GPU sweep (tests/test_gpu_voxelise_sweep.py) voxelises are sharp enough
to tell a subtly wrong kernel from a right one, fit the kernel's limits, and keep clear of denormals — and of the oracle
(oracle/voxel_oracle.py) on non-finite input."""
import warnings

import numpy as np
import pytest

import voxel_cases as vc
from oracle import voxel_oracle


def _oracle(case, gaussian):
    return voxel_oracle.voxelise(*case.cloud, case.V, case.edge, case.C, gaussian)


@pytest.fixture(scope="module")
def cases():
    return vc.one_launch_cases()


@pytest.mark.parametrize("V,edge,need_fma,need_reciprocal", [(21, 21.0, 20, None), (21, 20.0, 20, 20), (9, 12.5, 20, None)])
def test_face_cloud_tells_a_contracted_or_reciprocal_index_from_the_specified_one(V, edge, need_fma, need_reciprocal):
    """Spec item 3 asks for separate multiplies and adds, item 4 for a division.  A kernel that contracts the sums into FMAs, or
    multiplies by 1/a, moves atoms that sit on a voxel face into the neighbouring voxel.  With ~1500 atoms on faces the boolean
    frames of such a kernel differ from the specification's in at least 20 (voxel, channel) cells — measured for these generators:
    (21, 21.0) FMA 92, reciprocal 0; (21, 20.0) FMA 82, reciprocal 225; (9, 12.5) FMA 68, reciprocal 0.  At a = 1 the reciprocal is 1
    and that restatement IS the specification, so identity is asserted there; at (9, 12.5) the reciprocal happens to move no atom
    of this cloud and nothing is demanded of it."""
    cloud = vc.face_cloud(V, edge, 5, 1500, seed=V * 100 + int(edge))
    spec = vc.boolean_frames(cloud, V, edge, 5)
    assert np.array_equal(spec, voxel_oracle.voxelise(*cloud, V, edge, 5, False))         # the vectorised restatement is the oracle's
    fma = int(np.count_nonzero(vc.boolean_frames(cloud, V, edge, 5, "fma") != spec))
    rec = int(np.count_nonzero(vc.boolean_frames(cloud, V, edge, 5, "reciprocal") != spec))
    print(f"face_cloud V={V} edge={edge}: {int(spec.sum())} cells set; FMA differs in {fma} cells, reciprocal in {rec}")
    assert fma >= need_fma
    if vc.voxel_edge(V, edge) == 1.0:
        assert rec == 0                                  # by construction: x * (1 / 1) is x / 1
    elif need_reciprocal:
        assert rec >= need_reciprocal


def test_the_generators_put_their_atoms_where_they_say(cases):
    for V in (5, 21):
        for name, layers in ((f"interiors-{V}", "inner"), (f"borders-{V}", "outer")):
            case = cases[name]
            n_frames = len(case.cloud.frt)
            n = len(case.cloud.ch) // n_frames
            assert n_frames == (3 if layers == "outer" else 1)
            for r in range(n_frames):                    # frame r owns atoms r*n .. (r+1)*n
                _loc, idx, inside = voxel_oracle.locate(case.cloud.xyz[r * n:(r + 1) * n], case.cloud.frt[r], V, case.edge)
                assert inside.all()
                outer = np.any((idx == 0) | (idx == V - 1), axis=1)
                assert outer.all() if layers == "outer" else not outer.any()
    case = cases["borders-21"]
    _loc, idx, _in = voxel_oracle.locate(case.cloud.xyz[:150], case.cloud.frt[0], 21, case.edge)
    pinned = np.sum((idx == 0) | (idx == 20), axis=1)
    assert set(pinned.tolist()) == {1, 2, 3}             # faces, edges and corners
    case = cases["stacked-7"]
    _loc, idx, inside = voxel_oracle.locate(case.cloud.xyz, case.cloud.frt[0], case.V, case.edge)
    assert inside.all() and len({tuple(i) for i in idx.tolist()}) <= 4 and set(case.cloud.ch.tolist()) == {6}
    # the face cloud reaches one voxel beyond the cube on both sides, and channels -1 and C occur
    case = cases["sweep-bool-21-20.0-6"]
    loc, _idx, inside = voxel_oracle.locate(case.cloud.xyz[:600], case.cloud.frt[0], 21, 20.0)
    a = vc.voxel_edge(21, 20.0)
    assert loc.min() < -11.4 * a and loc.max() > 11.4 * a and 0.3 < inside.mean() < 0.9
    assert set(case.cloud.ch.tolist()) == set(range(-1, 7))


def test_chunked_cloud_fills_the_chunks_as_planned():
    for gaussian in (False, True):
        case, want = vc.chunking(gaussian)
        _loc, _idx, inside = voxel_oracle.locate(case.cloud.xyz, case.cloud.frt[0], case.V, case.edge)
        assert np.array_equal(inside, want) and len(want) == 5000
        per_chunk = [int(inside[b:b + vc.CHUNK].sum()) for b in range(0, 5000, vc.CHUNK)]
        assert len(per_chunk) == 20 and per_chunk.count(0) >= 4 and per_chunk[-1] > 0 and 5000 % vc.CHUNK != 0
        waves = inside[:19 * vc.CHUNK].reshape(-1, 64)
        assert waves.all(axis=1).sum() >= 4               # whole waves inside ...
        assert (~waves.any(axis=1)).sum() >= 16           # ... and whole waves outside
        assert inside.sum() <= (600 if gaussian else vc.MAX_LIST)


def test_every_cloud_fits_the_kernels_atom_list(cases):
    """at most 2048 encodable atoms inside each frame of a launch, by the oracle's own inside test; the capacity case exactly 2048"""
    for name, case in cases.items():
        ch_ok = (case.cloud.ch >= 0) & (case.cloud.ch < case.C)
        counts = [int((voxel_oracle.locate(case.cloud.xyz, row, case.V, case.edge)[2] & ch_ok).sum()) for row in case.cloud.frt]
        assert max(counts) <= vc.MAX_LIST, (name, max(counts))
        if name == "capacity-2048":
            assert counts == [vc.MAX_LIST, 10] and len(case.cloud.ch) == vc.MAX_LIST + 1500 + 10
            inside0 = voxel_oracle.locate(case.cloud.xyz, case.cloud.frt[0], 21, 21.0)[2]
            assert (inside0 & ~ch_ok).sum() > 500 and (~inside0).sum() > 300          # both kinds of atoms that must not count
    over = vc.capacity_cloud(vc.MAX_LIST + 1, 0, 71)
    assert [int(voxel_oracle.locate(over.xyz, row, 21, 21.0)[2].sum()) for row in over.frt] == [vc.MAX_LIST + 1, 10]


def test_no_gaussian_weight_is_near_the_denormal_range(cases):
    """sigma >= 0.25 a bounds the smallest of an atom's 27 weights by exp(-6.75 a^2 / (2 sigma^2)) = exp(-54) = 3.5e-24 before
    normalisation by a total of at most 27: no stored value is below 1e-30, so whether the GPU flushes denormals cannot change which
    voxels are non-zero."""
    for name, case in cases.items():
        assert np.all(case.cloud.sg >= np.float32(0.25) * np.float32(vc.voxel_edge(case.V, case.edge))), name
        if name.startswith(vc.GAUSSIAN_CASES) and not name.startswith("batch"):
            fr = _oracle(case, True)
            assert fr[fr != 0].min() >= 1e-30, name


def test_oracle_on_non_finite_input_encodes_the_finite_atoms_and_warns_of_nothing():
    cloud, normal, nan_frames = vc.nonfinite_cloud(90)
    assert np.isnan(cloud.xyz).sum() == 1 and np.isinf(cloud.xyz).sum() == 1 and (np.abs(cloud.xyz) == np.float32(1e20)).sum() == 1
    assert (cloud.xyz == np.float32(-3e9)).sum() == 1 and (~normal).sum() == 4 and nan_frames.sum() == 2
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for gaussian in (False, True):
            got = voxel_oracle.voxelise(*cloud, gaussian=gaussian)
            want = voxel_oracle.voxelise(*vc.subset(cloud, normal), gaussian=gaussian)
            assert not got[nan_frames].any() and got[~nan_frames].any(axis=(1, 2, 3, 4)).all()
            assert np.array_equal(got[~nan_frames], want[~nan_frames]) and not np.isnan(got).any()
        assert np.array_equal(vc.boolean_frames(cloud, 21, 21.0, 5), voxel_oracle.voxelise(*cloud, gaussian=False))
        _loc, idx, inside = voxel_oracle.locate(cloud.xyz, cloud.frt[3])
        assert not inside.any() and not idx.any()


def test_recorded_digests_cover_the_cases_and_say_where_they_come_from():
    """tests/golden/voxelise_digests.json: one entry per case of digest_cases and the frames of 1ubq, each of the shape the case's
    cloud and geometry give, recorded at the last commit at which th_voxelise had a kernel of its own"""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "voxelise_digests.json")) as f:
        rec = json.load(f)
    assert rec["commit"] == "51dee49" and rec["hip"] and "gfx950" in rec["device"]
    calls = vc.digest_cases()
    assert list(rec["cases"]) == [c[0] for c in calls] + [vc.UBQ_DIGEST] and len(set(rec["cases"])) == 69
    for case_id, cloud, V, edge, C, gaussian in calls:
        got = rec["cases"][case_id]
        assert got["shape"] == [len(cloud.frt), V, V, V, C] and got["dtype"] == ("float32" if gaussian else "uint8"), case_id
        assert len(got["sha256"]) == 64
    assert rec["cases"][vc.UBQ_DIGEST]["shape"] == [76, 21, 21, 21, 5]
