"""th_tag_rotamers on the GPU: rotamer classes equal, AS BYTES, to the committed fixture of 1ubq and to the NumPy restatement
(tests/rotamer_restatement.py) on seeded synthetic residues of all 20 types; the bin edges; every way a residue stays unlabelled;
batching and repeatability; ABI errors; tag_pdb_with_rot, tag_rotamers.py and analyse_rotamers.py --path_to_pdb end to end.

Classes are integers and must be exact.  The chi angles have a MEASURED tolerance: the float64 restatement's own worst error
against the same formula in np.longdouble is measured on the data of the test, and the GPU is allowed 64 times that (the margin
covers a device atan2 / sqrt that is a few ulp off and, were the compiler to contract them, fused cross products).

Each test prints its figures before it asserts; profiles/rotamer_tags.txt records them.
"""
import csv
import ctypes as C
import json
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rotamer_restatement as rr  # noqa: E402
from timed_hip import _lib, pdbio, structure  # noqa: E402

pytestmark = pytest.mark.gpu

MARGIN = 64


@pytest.fixture(scope="module")
def golden():
    return np.load(rr.GOLDEN)


@pytest.fixture(scope="module")
def ubq():
    return rr.residues_of_model(pdbio.read_pdb(rr.UBQ)[0])


@pytest.fixture(scope="module")
def synthetic():
    residues = rr.synthetic_residues()
    cls, chi = rr.restate(residues)
    _, exact = rr.restate(residues, dtype=np.longdouble)
    return residues, cls, chi, exact


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def tag(residues, gpu, **kw):
    return structure.rotamer_classes(*rr.flatten(residues), device=gpu, **kw)


def check_chi(what, got, float64, exact):
    """the measured tolerance of the module docstring; NaN in the same places"""
    assert np.array_equal(np.isnan(got), np.isnan(float64)), what
    own = float(np.nanmax(np.abs(float64.astype(np.longdouble) - exact)))
    mine = float(np.nanmax(np.abs(got.astype(np.longdouble) - exact)))
    print(f"{what}: {int(np.isfinite(got).sum())} angles; float64 restatement vs long double {own:.3e} degrees, GPU vs long double {mine:.3e}, "
          f"allowed {MARGIN * own:.3e}")
    assert own > 0 and mine <= MARGIN * own, (what, own, mine)


def test_1ubq_classes_equal_the_fixture_as_bytes(gpu, golden, ubq):
    assert rr.coords_sha256(ubq) == str(golden["sha256"])
    cls, chi = tag(ubq, gpu)
    print("1ubq residues", len(cls), "differing classes", int((cls != golden["cls"]).sum()))
    assert same_bytes(cls, golden["cls"])
    _, exact = rr.restate(ubq, dtype=np.longdouble)
    check_chi("1ubq", chi, golden["chi"], exact)
    only, none = tag(ubq, gpu, chi=False)                       # chi_out is optional
    assert none is None and same_bytes(only, cls)
    (tagged,) = structure.tag_rotamers([rr.UBQ], device=gpu)
    assert same_bytes(tagged.cls, golden["cls"]) and same_bytes(tagged.chi, chi) and len(tagged.residues) == 76
    assert tagged.rotamers[:3] == ["122", "223", "12"]                     # MET 158 + 4, GLN 203 + 14, ILE 59 + 1


def test_synthetic_residues_of_all_types_equal_the_restatement(gpu, synthetic):
    residues, want, chi64, exact = synthetic
    assert {res for res, _ in residues} == set(rr.RESIDUES) and len(residues) == 400
    assert rr.edge_distance(chi64) > 1e-6                       # no generated angle sits on a bin edge: nothing is dropped
    assert (want >= 0).all() and len(set(want.tolist())) > 120
    assert sum(len({n for n, _ in atoms}) < len(atoms) for _, atoms in residues) > 100          # duplicate names, the first wins
    cls, chi = tag(residues, gpu)
    print("synthetic residues", len(cls), "differing classes", int((cls != want).sum()))
    assert same_bytes(cls, want)
    check_chi("synthetic", chi, chi64, exact)


def _serine(n_y, og_y):
    return ("SER", [("N", np.array([-0.5, n_y, 0.0])), ("CA", np.zeros(3)), ("CB", np.array([1.5, 0.0, 0.0])), ("OG", np.array([2.0, og_y, 0.0]))])


def test_bin_edges(gpu):
    ser = rr.CLASS_BASE["SER"]
    planar = [_serine(1.0, 1.0), _serine(-1.0, -1.0), _serine(1.0, -1.0), _serine(-1.0, 1.0)]
    zigzag = ("ARG", [(name, np.array([1.2 * k, 0.7 * (k % 2), 0.0])) for k, name in enumerate(rr.path_of("ARG"))])
    cls, chi = tag(planar + [zigzag], gpu)
    print("planar chi", chi[:4, 0].tolist(), chi[4].tolist())
    assert cls.tolist() == [ser, ser, ser + 1, ser + 1, rr.CLASS_BASE["ARG"] + 27 + 9 + 3 + 1]       # cis: bin 1; trans: bin 2, either sign
    assert (np.abs(chi[:2, 0]) < 1e-9).all() and (np.abs(np.abs(chi[2:4, 0]) - 180.0) < 1e-9).all() and (np.abs(np.abs(chi[4]) - 180.0) < 1e-9).all()
    near = [rr.serine_at(t) for t in (120 - 1e-3, 120 + 1e-3, -120 + 1e-3, -120 - 1e-3)]
    want, want_chi = rr.restate(near)
    assert np.abs(np.abs(want_chi[:, 0]) - 120.0).max() < 1.1e-3 and np.abs(np.abs(want_chi[:, 0]) - 120.0).min() > 0.9e-3
    assert want.tolist() == [ser, ser + 1, ser + 2, ser + 1]
    cls, chi = tag(near, gpu)
    assert same_bytes(cls, want) and np.abs(chi[:, 0] - want_chi[:, 0]).max() < 1e-9


def test_unlabelled_residues(gpu, lib):
    rng = np.random.default_rng(3)

    def full(res, drop=(), nan_on=None):
        atoms = [(n, np.round(rng.uniform(-4, 4, 3), 3)) for n in (rr.path_of(res) or ("N", "CA")) + ("C", "O") if n not in drop]
        if nan_on:
            atoms = [(n, np.array([p[0], np.nan, p[2]]) if n == nan_on else p) for n, p in atoms]
        return (res, atoms)
    residues = [full("LEU"), ("MSE", full("MET")[1]), ("HOH", [("O", np.zeros(3))]), full("SER", drop=("CB",)), full("LYS", drop=("NZ",)),
                full("ARG", nan_on="CD"), full("ALA"), full("GLY"), ("LEU", []), ("GLY", []), full("ARG", nan_on="O"), full("TRP")]
    want, want_chi = rr.restate(residues)
    labelled = [True, False, False, False, False, False, True, True, False, True, True, True]
    assert ((want >= 0) == np.array(labelled)).all()
    cls, chi = tag(residues, gpu)
    assert same_bytes(cls, want) and np.array_equal(np.isnan(chi), np.isnan(want_chi))
    assert np.isnan(chi[~np.array(labelled)]).all()                         # the chi of an unlabelled residue stays NaN
    assert cls[6] == rr.CLASS_BASE["ALA"] and cls[7] == cls[9] == rr.CLASS_BASE["GLY"]
    flagged, _ = tag(residues, gpu, ala_gly_class=False)                    # flag bit 0
    assert same_bytes(flagged, rr.restate(residues, ala_gly_class=False)[0])
    assert flagged[[6, 7, 9]].tolist() == [-1, -1, -1] and same_bytes(np.delete(flagged, [6, 7, 9]), np.delete(cls, [6, 7, 9]))
    # only residues without atoms: nothing to copy in, still labelled by type
    cls, chi = structure.rotamer_classes(np.zeros((0, 3)), np.zeros(0, np.uint32), [0, 0, 0], [5, 9], device=gpu)
    assert cls.tolist() == [rr.CLASS_BASE["GLY"], -1] and np.isnan(chi).all()
    # n_res == 0
    cls, chi = structure.rotamer_classes(np.zeros((0, 3)), np.zeros(0, np.uint32), [0], [], device=gpu)
    assert cls.shape == (0,) and chi.shape == (0, 4)
    assert lib.th_tag_rotamers(gpu, None, None, 0, None, None, 0, 0, None, None, None) == _lib.TH_OK
    assert structure.tag_rotamers([], device=gpu) == []
    (empty,) = structure.tag_rotamers([pdbio.Model(1, [])], device=gpu)
    assert empty.cls.shape == (0,) and empty.chi.shape == (0, 4) and empty.residues == []


def _model_of(residues, chain="A"):
    """a pdbio.Model of restatement residues (a dict keeps the first atom of a name, as pdbio does)"""
    out = []
    for k, (res, atoms) in enumerate(residues):
        first = {}
        for name, pos in atoms:
            first.setdefault(name, pos)
        out.append(pdbio.Residue(chain, str(k + 1), res, atoms=first))
    return pdbio.Model(1, out)


def test_batches_cut_by_a_tiny_budget_give_the_same_bytes(gpu, golden, synthetic):
    residues, want, _, _ = synthetic
    ubq_model = pdbio.read_pdb(rr.UBQ)[0]
    structures = [ubq_model, _model_of(residues[:150]), pdbio.Model(1, []), _model_of(residues[150:151]), ubq_model, _model_of(residues[151:])]
    stats = {}
    whole = structure.tag_rotamers(structures, device=gpu, stats=stats)
    assert stats["submissions"] == 1
    sizes = [sum(len(r.atoms) for r in structure.first_model(s).residues if not r.hetero) for s in structures]
    budget = 700 * structure._ATOM_BYTES
    runs = structure.cut_batches(sizes, budget)
    assert len(runs) >= 4
    stats = {}
    split = structure.tag_rotamers(structures, device=gpu, budget_bytes=budget, stats=stats)
    assert stats["submissions"] == len(runs)
    again = structure.tag_rotamers(structures, device=gpu)
    for a, b, c in zip(whole, split, again):
        assert same_bytes(a.cls, b.cls) and same_bytes(a.chi, b.chi) and same_bytes(a.cls, c.cls) and same_bytes(a.chi, c.chi)
    assert same_bytes(whole[0].cls, golden["cls"]) and same_bytes(whole[4].cls, golden["cls"])
    assert same_bytes(np.concatenate([whole[1].cls, whole[3].cls, whole[5].cls]), want)


def _raw_call(lib, xyz, names, total, offsets, types, n_res, cls, chi):
    def ptr(a):
        return None if a is None else a.ctypes.data_as(C.c_void_p)
    return lib.th_tag_rotamers(0, ptr(xyz), ptr(names), total, ptr(offsets), ptr(types), n_res, 0, ptr(cls), ptr(chi), None)


def test_abi_errors_return_einval_and_leave_the_outputs_untouched(gpu, lib, ubq):
    xyz, names, offsets, types = rr.flatten(ubq[:3])
    total = len(xyz)
    decreasing = offsets.copy()
    decreasing[2] = decreasing[1] - 1
    past = offsets.copy()
    past[-1] = total + 1
    below = offsets.copy()
    below[0] = -1
    bad_calls = {
        "offsets decrease": dict(offsets=decreasing),
        "negative total": dict(total=-1),
        "negative n_res": dict(n_res=-1),
        "cls_out NULL": dict(cls=None),
        "offsets NULL": dict(offsets=None),
        "types NULL": dict(types=None),
        "xyz NULL": dict(xyz=None),
        "names NULL": dict(names=None),
        "offsets past total": dict(offsets=past),
        "offsets below zero": dict(offsets=below),
        "type 20": dict(types=np.array([20, 0, 0], np.int8)),
        "type -2": dict(types=np.array([0, -2, 0], np.int8)),
    }
    for what, change in bad_calls.items():
        cls = np.full(3, 12345, np.int16)
        chi = np.full((3, 4), 6.5)
        kw = dict(xyz=xyz, names=names, total=total, offsets=offsets, types=types, n_res=3, cls=cls, chi=chi)
        kw.update(change)
        assert _raw_call(lib, **kw) == _lib.TH_EINVAL, what
        assert b"th_tag_rotamers" in lib.th_last_error(), what
        assert (cls == 12345).all() and (chi == 6.5).all(), what
    cls = np.full(3, 12345, np.int16)
    chi = np.full((3, 4), 6.5)
    assert _raw_call(lib, xyz, names, total, offsets, types, 3, cls, chi) == _lib.TH_OK
    assert same_bytes(cls, rr.restate(ubq[:3])[0])
    with pytest.raises(_lib.TimedHipError) as err:
        structure.rotamer_classes(xyz, names, [0, 9, 8, total], types, device=gpu)
    assert err.value.code == _lib.TH_EINVAL


def test_tag_pdb_with_rot_and_tag_rotamers_cli(gpu, golden, tmp_path, capsys):
    from design_utils import analyse_utils as au
    import tag_rotamers
    root = tmp_path / "pdb"
    (root / "ub").mkdir(parents=True)
    shutil.copy(rr.UBQ, root / "ub" / "1ubq.pdb1.gz")
    results, assemblies = au.tag_pdb_with_rot(4, root, np.array(["1ubqA", "2xyzA"]), device=gpu)
    assert "Could not find" in capsys.readouterr().out
    assert results == {"1ubqA": golden["cls"].tolist()} and assemblies["1ubq"]["A"].sequence.startswith("MQIFVKTLTGK")
    out = tmp_path / "out"
    tag_rotamers.main(tag_rotamers.build_parser().parse_args(["--path_to_pdb", str(root), "--path_to_output", str(out), "--device", str(gpu)]))
    assert "in 1 GPU submission(s)" in capsys.readouterr().out
    assert json.loads((out / "rotamer_labels.json").read_text()) == {"1ubqA": golden["cls"].tolist()}
    with open(out / "chi_angles.csv", newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["structure", "chain", "residue", "name", "chi1", "chi2", "chi3", "chi4", "rotamer", "class"] and len(rows) == 77
    assert rows[1][:4] == ["ub/1ubq.pdb1.gz", "A", "1", "MET"] and rows[1][7:] == ["", "122", "162"]
    chi = np.array([[float(x) if x else np.nan for x in r[4:8]] for r in rows[1:]])
    assert np.array_equal(np.isnan(chi), np.isnan(golden["chi"])) and np.nanmax(np.abs(chi - golden["chi"])) < 1e-9
    assert [int(r[9]) for r in rows[1:]] == golden["cls"].tolist()


def test_analyse_rotamers_from_structures_equals_the_run_fed_its_labels_file(gpu, golden, tmp_path):
    import analyse_rotamers
    root = tmp_path / "pdb"
    (root / "ub").mkdir(parents=True)
    shutil.copy(rr.UBQ, root / "ub" / "1ubq.pdb1.gz")
    rng = np.random.default_rng(8)
    probs = rng.dirichlet(np.full(338, 0.05), 76)
    truth = golden["cls"]
    probs[np.arange(0, 76, 2), truth[::2]] += 0.5                     # a model that is right half of the time
    np.savetxt(tmp_path / "M_rot.csv", probs.astype(np.float16), delimiter=",")
    (tmp_path / "map.txt").write_text("ignore_uncommon False\ninclude_pdbs\n##########\n1ubqA 76\n")
    common = ["--path_to_pred_matrix", str(tmp_path / "M_rot.csv"), "--path_to_datasetmap", str(tmp_path / "map.txt"), "--device", str(gpu)]
    tagged = analyse_rotamers.main(analyse_rotamers.build_parser().parse_args(common + ["--output_path", str(tmp_path / "a"), "--path_to_pdb", str(root)]))
    labels = tmp_path / "a_M_rot" / "rotamer_labels.json"
    assert json.loads(labels.read_text()) == {"1ubqA": truth.tolist()}
    fed = analyse_rotamers.main(analyse_rotamers.build_parser().parse_args(common + ["--output_path", str(tmp_path / "b"), "--path_to_rotamer_labels", str(labels)]))
    assert tagged == fed and tagged["n_labelled"] == 76 and tagged["accuracy_1"] >= 0.5
    name = "results_M_rot_vs_original.json"
    assert (tmp_path / "a_M_rot" / name).read_bytes() == (tmp_path / "b_M_rot" / name).read_bytes()
