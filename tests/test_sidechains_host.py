"""th_build_sidechains without a GPU: the table against the restatement's own copy of the tree, row for row, and against the chi
paths of th_rotamer_table; the table checked by data (1ubq rebuilt from its native chi angles) and by ring closure and planarity;
class -> centre angles for all 338 classes; write_pdb / read_pdb; batching cuts; argument errors (which are found before any
device is touched)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rotamer_restatement as rr  # noqa: E402
import sidechain_restatement as sr  # noqa: E402
from timed_hip import _lib, pdbio, sidechains, structure  # noqa: E402

RMSD_BOUND = 0.40            # Angstrom: the per-type means of 1ubq itself give 0.331; the margin is for standard values
CLOSURE_BOUND = 0.05
PLANAR_BOUND = 0.02


@pytest.fixture(scope="module")
def golden():
    return np.load(sr.GOLDEN)


@pytest.fixture(scope="module")
def ubq():
    return sr.ubq_inputs()


def test_table_equals_the_restatement_row_for_row(lib):
    table = sidechains.sidechain_table()
    assert [t.res for t in table] == rr.RESIDUES == list(sr.TREE)
    for t in table:
        rows = sr.TREE[t.res]
        assert t.atoms == tuple(row[0] for row in rows), t.res
        assert t.parents == tuple(row[1] for row in rows), t.res
        assert t.chi_index == tuple(row[2] for row in rows), t.res
        assert t.geometry == tuple(tuple(float(x) for x in row[3:6]) for row in rows), t.res
        assert t.closure == tuple(sr.CLOSURE.get(t.res, ())), t.res
        for j, (a, b, c) in enumerate(t.parents):                          # a parent comes before its child
            assert all(p in ("N", "CA", "C") + t.atoms[:j] for p in (a, b, c)), (t.res, t.atoms[j])
    assert max(len(t.atoms) for t in table) == sidechains.MAX_ATOMS == 10 and table[rr.RESIDUES.index("GLY")].atoms == ()
    assert all(t.atoms[0] == "CB" and t.parents[0] == ("C", "N", "CA") and t.chi_index[0] == -1 for t in table if t.atoms)


def test_every_chi_path_atom_is_built_at_its_chi_angle(lib):
    table = {t.res: t for t in sidechains.sidechain_table()}
    for res, n_chi, _, path in structure.rotamer_table():
        assert n_chi == sr.n_chi_needed(res)
        t = table[res]
        for k in range(n_chi):
            j = t.atoms.index(path[k + 3])
            assert t.parents[j] == tuple(path[k:k + 3]) and t.chi_index[j] == k and t.geometry[j][2] == 0.0, (res, path[k + 3])


def test_table_rebuilds_1ubq_within_the_bound(golden, ubq):
    residues, natives, sha = ubq
    assert sha == str(golden["sha256"])
    xyz, n_built = sr.restate_build(residues)
    n_matched, sum_sq = sr.restate_match(residues, xyz, n_built, natives)
    rmsd = sr.overall_rmsd(n_matched, sum_sq)
    print(f"1ubq from native chi: {int((n_built > 0).sum())} residues, {int(n_matched.sum())} atoms, RMSD {rmsd:.4f} (stored {float(golden['rmsd']):.4f})")
    assert int((n_built > 0).sum()) == 70 and int(n_matched.sum()) == 297
    assert rmsd <= RMSD_BOUND and abs(rmsd - float(golden["rmsd"])) < 1e-9
    assert np.array_equal(n_built, golden["n_built"]) and np.array_equal(n_matched, golden["n_matched"])
    assert np.allclose(xyz, golden["xyz"], rtol=0, atol=1e-9, equal_nan=True)


def test_rings_close_and_are_planar():
    closures, planar = sr.closure_and_planarity()
    assert sorted({c[0] for c in closures}) == ["HIS", "PHE", "TRP", "TYR"] and len(closures) == 5
    for res, a, b, stated, got in closures:
        print(f"{res} {a}-{b}: stated {stated}, built {got:.4f}")
        assert abs(got - stated) <= CLOSURE_BOUND, (res, a, b)
    print("planarity", planar)
    assert max(planar.values()) <= PLANAR_BOUND


def test_place_gives_the_dihedral_it_was_asked_for():
    rng = np.random.default_rng(2)
    for _ in range(50):
        a, b, c = rng.normal(size=(3, 3)) * 2.0
        length, theta, phi = rng.uniform(1.0, 2.0), rng.uniform(95.0, 135.0), rng.uniform(-179.0, 179.0)
        d = sr.place(a, b, c, length, theta, phi)
        u, v = b - c, d - c
        assert abs(rr.dihedral(a, b, c, d) - phi) < 1e-9 and abs(np.linalg.norm(v) - length) < 1e-12
        assert abs(np.degrees(np.arccos(u @ v / np.linalg.norm(u) / np.linalg.norm(v))) - theta) < 1e-9


def test_class_centres_of_all_338_classes(lib):
    classes = np.arange(rr.N_CLASSES)
    types, chi = sidechains.class_centres(classes)
    assert rr.N_CLASSES == 338 and types.dtype == np.int8 and chi.shape == (338, 4)
    for c in classes:
        res, want = sr.class_centres(int(c))
        assert rr.RESIDUES[types[c]] == res and np.array_equal(chi[c], want, equal_nan=True), c
        angles = want[np.isfinite(want)]
        assert len(angles) == len(rr.TAILS[res]) and set(angles.tolist()) <= {60.0, 180.0, -60.0}
        # the centres tag back to the class they came from (the restatement's bins)
        index = 0
        for x in angles:
            index = index * 3 + (rr.bin_of(x if x < 180.0 else -180.0) - 1)
        assert rr.CLASS_BASE[res] + index == c
    types, chi = sidechains.class_centres([-1, 0])
    assert types.tolist() == [-1, 0] and np.isnan(chi).all()
    with pytest.raises(ValueError):
        sidechains.class_centres([338])


def test_write_pdb_read_pdb_round_trip(tmp_path):
    model = pdbio.read_pdb(rr.UBQ)[0]
    rng = np.random.default_rng(4)
    extra = pdbio.Residue("B", "100A", "TRP", atoms={n: rng.uniform(-999.0, 999.0, 3) for n in ("N", "CA", "CH2", "1HD1", "HD11")},
                          bfactors={"N": 12.345, "CA": float("nan")})
    ion = pdbio.Residue("B", "201", "CA", atoms={"CA": np.array([1.0, -2.0, 3.0004])}, elements={"CA": "CA"}, hetero=True)
    model = pdbio.Model(1, [r for r in model.residues if not r.hetero] + [extra, ion])
    for path in (tmp_path / "out.pdb", tmp_path / "out.pdb.gz"):
        n = pdbio.write_pdb(path, model)
        assert n == sum(len(r.atoms) for r in model.residues)
        (back,) = pdbio.read_pdb(path)
        assert [(r.chain, r.number, r.name, r.hetero) for r in back.residues] == [(r.chain, r.number, r.name, r.hetero) for r in model.residues]
        for a, b in zip(model.residues, back.residues):
            assert list(a.atoms) == list(b.atoms)
            for name in a.atoms:
                assert np.array_equal(np.round(a.atoms[name], 3), b.atoms[name]), (a.name, name)
        assert back.residues[-2].bfactors["N"] == 12.35 or back.residues[-2].bfactors["N"] == 12.34
        assert back.residues[-2].bfactors["CA"] == 0.0 and back.residues[-2].bfactors["CH2"] == 0.0
        assert back.residues[0].bfactors == model.residues[0].bfactors
        assert back.residues[-1].elements["CA"] == "CA" and back.residues[-2].elements["CA"] == "C" and back.residues[-2].elements["1HD1"] == "H"
    lines = (tmp_path / "out.pdb").read_text().splitlines()
    assert lines[0] == "ATOM      1  N   MET A   1      27.340  24.430   2.614  1.00  9.67           N"
    assert lines[-1] == "END" and [l[:3] for l in lines].count("TER") == 2 and all(len(l) == 78 for l in lines if l.startswith(("ATOM", "HETATM")))
    ch2 = next(l for l in lines if l[12:16] == " CH2")
    hd = next(l for l in lines if l[12:16] == "1HD1")
    ca = next(l for l in lines if l.startswith("HETATM"))
    assert ch2[17:27] == "TRP B 100A" and hd[76:78] == " H" and ca[12:16] == "CA  " and ca[76:78] == "CA"


def test_matrix_rows_pair_with_residues_by_chain_and_number():
    import build_sidechains
    layout = structure.rotamer_layout(pdbio.read_pdb(rr.UBQ)[0])
    rows = [["1ubq", "A", " 3", "I"], ["1UBQ", "A", "999", "X"], ["2xyz", "A", "3", "I"], ["1ubq", "B", "3", "I"], ["1ubq", "A", "1", "M"]]
    matrix = np.zeros((5, 338))
    matrix[np.arange(5), [60, 61, 62, 63, 160]] = 1.0
    ((cls, unmatched),) = build_sidechains.classes_from_matrix(matrix, rows, ["ub/1ubq.pdb1.gz"], [layout])
    assert unmatched == 2 and cls[2] == 60 and cls[0] == 160 and (np.delete(cls, [0, 2]) == -1).all() and cls.dtype == np.int16
    with pytest.raises(ValueError):
        build_sidechains.classes_from_matrix(matrix, rows[:4], ["ub/1ubq.pdb1.gz"], [layout])
    with pytest.raises(ValueError):
        build_sidechains.classes_from_matrix(matrix[:2], [["1ubqA", "76"], ["2xyzA", "10"]], ["ub/1ubq.pdb1.gz"], [layout])


def test_batching_cuts():
    assert sidechains.cut_batches([76, 76, 76], 10 ** 9) == [(0, 3)]
    assert sidechains.cut_batches([76, 76, 76], 100 * sidechains._RES_BYTES) == [(0, 1), (1, 2), (2, 3)]
    assert sidechains.cut_batches([10, 0, 20, 500, 5], 40 * sidechains._RES_BYTES) == [(0, 3), (3, 4), (4, 5)]
    assert sidechains.cut_batches([], 1) == []


def _call(lib, **change):
    """th_build_sidechains on three residues with one argument changed; the outputs must stay untouched"""
    kw = dict(backbone=np.zeros((3, 3, 3)), types=np.array([0, 1, 2], np.int8), chi=np.zeros((3, 4)), chain=None,
              offsets=np.array([0, 2, 3], np.int64), n_struct=2, n_res=3, n_xyz=None, n_name=None, n_total=0, n_off=None, n_type=None,
              distance=2.5, flags=0, xyz=np.full((3, 10, 3), 7.5), built=np.full(3, 77, np.int32), matched=None, sum_sq=None,
              clashes=np.full(3, 77, np.int32), pairs=np.full(2, 77, np.int64))
    kw.update(change)
    p = _lib.ptr
    rc = lib.th_build_sidechains(0, p(kw["backbone"]), p(kw["types"]), p(kw["chi"]), p(kw["chain"]), p(kw["offsets"]), kw["n_struct"], kw["n_res"],
                                 p(kw["n_xyz"]), p(kw["n_name"]), kw["n_total"], p(kw["n_off"]), p(kw["n_type"]), kw["distance"], kw["flags"],
                                 p(kw["xyz"]), p(kw["built"]), p(kw["matched"]), p(kw["sum_sq"]), p(kw["clashes"]), p(kw["pairs"]), None)
    untouched = all((kw[k] == v).all() for k, v in (("xyz", 7.5), ("built", 77), ("clashes", 77), ("pairs", 77)) if kw[k] is not None)
    return rc, untouched


BAD_CALLS = {
    "negative n_res": dict(n_res=-1),
    "negative n_struct": dict(n_struct=-1),
    "too many residues": dict(n_res=2 ** 31),
    "offsets do not end at n_res": dict(n_res=2),
    "offsets do not start at 0": dict(offsets=np.array([1, 2, 3], np.int64)),
    "offsets decrease": dict(offsets=np.array([0, 4, 3], np.int64)),
    "offsets NULL": dict(offsets=None),
    "type 20": dict(types=np.array([0, 20, 2], np.int8)),
    "type -2": dict(types=np.array([-2, 1, 2], np.int8)),
    "backbone NULL": dict(backbone=None),
    "chi NULL": dict(chi=None),
    "out_xyz NULL": dict(xyz=None),
    "out_n_built NULL": dict(built=None),
    "unknown flag": dict(flags=2),
    "clash distance 0": dict(distance=0.0),
    "clash distance NaN": dict(distance=float("nan")),
    "native outputs without a native": dict(matched=np.zeros(3, np.int32), sum_sq=np.zeros(3)),
    "native without its outputs": dict(n_off=np.zeros(4, np.int64), n_type=np.zeros(3, np.int8)),
    "native offsets past total": dict(n_off=np.array([0, 0, 0, 1], np.int64), n_type=np.zeros(3, np.int8), matched=np.zeros(3, np.int32), sum_sq=np.zeros(3)),
    "native offsets decrease": dict(n_off=np.array([0, 1, 0, 1], np.int64), n_type=np.zeros(3, np.int8), matched=np.zeros(3, np.int32), sum_sq=np.zeros(3),
                                    n_total=1, n_xyz=np.zeros((1, 3)), n_name=np.zeros(1, np.uint32)),
    "native type 20": dict(n_off=np.zeros(4, np.int64), n_type=np.array([0, 0, 20], np.int8), matched=np.zeros(3, np.int32), sum_sq=np.zeros(3)),
    "n_struct 0 with residues": dict(n_struct=0),
}


@pytest.mark.parametrize("what", list(BAD_CALLS))
def test_abi_errors_are_found_before_any_device_is_touched(lib, what):
    rc, untouched = _call(lib, **BAD_CALLS[what])
    assert rc == _lib.TH_EINVAL and b"th_build_sidechains" in lib.th_last_error() and untouched, what


def test_empty_calls_and_python_argument_errors(lib):
    assert lib.th_build_sidechains(0, None, None, None, None, None, 0, 0, None, None, 0, None, None, 2.5, 0, None, None, None, None, None, None, None) == _lib.TH_OK
    pairs = np.full(2, 77, np.int64)
    rc, _ = _call(lib, n_res=0, offsets=np.zeros(3, np.int64), pairs=pairs, backbone=None, types=None, chi=None, xyz=None, built=None, clashes=None)
    assert rc == _lib.TH_OK and pairs.tolist() == [0, 0]                          # only empty structures: nothing is launched
    assert lib.th_sidechain_table(20, None, None, None, None, None, None, None, None) == _lib.TH_EINVAL and b"th_sidechain_table" in lib.th_last_error()
    assert lib.th_sidechain_table(18, None, None, None, None, None, None, None, None) == _lib.TH_OK
    n = C.c_int(0)
    assert lib.th_sidechain_table(5, C.byref(n), None, None, None, None, None, None, None) == _lib.TH_OK and n.value == 0
    with pytest.raises(ValueError):
        sidechains.build_arrays(np.zeros((3, 2, 3)), [0, 1, 2], np.zeros((3, 4)))
    with pytest.raises(ValueError):
        sidechains.build_arrays(np.zeros((3, 3, 3)), [0, 1, 2], np.zeros((2, 4)))
    with pytest.raises(ValueError):
        sidechains.build_arrays(np.zeros((3, 3, 3)), [0, 1, 2], np.zeros((3, 4)), chain_id=[0, 0])
    with pytest.raises(ValueError):
        sidechains.build_arrays(np.zeros((3, 3, 3)), [0, 1, 2], np.zeros((3, 4)), native=(np.zeros((2, 3)), np.zeros(2), [0, 1, 2], [0, 1, 2]))
    with pytest.raises(_lib.TimedHipError) as err:
        sidechains.build_arrays(np.zeros((3, 3, 3)), [0, 1, 2], np.zeros((3, 4)), struct_offsets=[0, 2])
    assert err.value.code == _lib.TH_EINVAL
    with pytest.raises(ValueError):
        sidechains.build([], chi="scwrl")
    assert sidechains.build([], chi="class_centres", classes=[]) == []
