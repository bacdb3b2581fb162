"""th_build_sidechains on the GPU against the NumPy restatement (tests/sidechain_restatement.py) and the committed fixture of 1ubq:
built coordinates, the deviation from the native, clash counts as exact integers, every way a residue stays unbuilt, the round trip
through th_tag_rotamers for all 338 classes, batching and repeatability, ABI errors, build_sidechains.py end to end.

Coordinates have a MEASURED tolerance, the rule and the margin of tests/test_gpu_rotamers.py: the float64 restatement's own worst
error against the same formulas in np.longdouble is measured on the data of the test, and the GPU is allowed 64 times that (the
margin covers a device sin / cos / sqrt that is a few ulp off and, were the compiler to contract them, fused cross products).
Counts are integers and must be equal as bytes.

Each test prints its figures before it asserts; profiles/sidechains.txt records them.
"""
import csv
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rotamer_restatement as rr  # noqa: E402
import sidechain_restatement as sr  # noqa: E402
from test_sidechains_host import BAD_CALLS, _call  # noqa: E402
from timed_hip import _lib, pdbio, sidechains, structure  # noqa: E402

pytestmark = pytest.mark.gpu

MARGIN = 64
RMSD_BOUND = 0.40


@pytest.fixture(scope="module")
def golden():
    return np.load(sr.GOLDEN)


@pytest.fixture(scope="module")
def ubq():
    return sr.ubq_inputs()


@pytest.fixture(scope="module")
def synthetic():
    residues = sr.synthetic_residues()
    xyz, n_built = sr.restate_build(residues)
    exact, _ = sr.restate_build(residues, dtype=np.longdouble)
    return residues, xyz, n_built, exact


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def arrays(residues):
    """restatement residues as build_arrays takes them: backbone, types, chi"""
    nb = len(residues[0][1]) if residues else 3
    return (np.array([r[1] for r in residues], dtype=np.float64).reshape(-1, nb, 3), np.array([sr.type_index(r[0]) for r in residues], dtype=np.int8),
            np.array([r[2] for r in residues], dtype=np.float64).reshape(-1, 4))


def check_xyz(what, got, float64, exact):
    """the measured tolerance of the module docstring; NaN in the same places"""
    assert np.array_equal(np.isnan(got), np.isnan(float64)), what
    own = float(np.nanmax(np.abs(float64.astype(np.longdouble) - exact)))
    mine = float(np.nanmax(np.abs(got.astype(np.longdouble) - exact)))
    print(f"{what}: {int(np.isfinite(got).sum()) // 3} atoms; float64 restatement vs long double {own:.3e} Angstrom, GPU vs long double {mine:.3e}, "
          f"allowed {MARGIN * own:.3e}")
    assert own > 0 and mine <= MARGIN * own, (what, own, mine)


def test_1ubq_from_native_chi_equals_the_fixture(gpu, golden, ubq):
    residues, natives, sha = ubq
    assert sha == str(golden["sha256"])
    backbone, types, chi = arrays(residues)
    got = sidechains.build_arrays(backbone, types, chi, native=rr.flatten(natives), device=gpu)
    exact, _ = sr.restate_build(residues, dtype=np.longdouble)
    check_xyz("1ubq", got.xyz, golden["xyz"], exact)
    assert same_bytes(got.n_built, golden["n_built"]) and same_bytes(got.n_matched, golden["n_matched"])
    _, exact_sq = sr.restate_match(residues, exact, golden["n_built"], natives, dtype=np.longdouble)
    on = golden["n_matched"] > 0
    own = float(np.max(np.abs(golden["sum_sq"][on].astype(np.longdouble) - exact_sq[on]) / exact_sq[on]))
    mine = float(np.max(np.abs(got.sum_sq[on].astype(np.longdouble) - exact_sq[on]) / exact_sq[on]))
    print(f"1ubq sum_sq: float64 restatement vs long double {own:.3e} relative, GPU vs long double {mine:.3e}, allowed {MARGIN * own:.3e}")
    assert own > 0 and mine <= MARGIN * own and (got.sum_sq[~on] == 0).all()
    rmsd = float(np.sqrt(got.sum_sq.sum() / got.n_matched.sum()))
    print(f"1ubq: {int((got.n_built > 0).sum())} residues built, {int(got.n_matched.sum())} atoms matched, RMSD {rmsd:.4f} Angstrom, "
          f"{int(got.pairs[0])} clashing pairs")
    assert int(got.n_matched.sum()) == 297 and rmsd <= RMSD_BOUND
    assert same_bytes(got.clashes, golden["clashes"]) and same_bytes(got.pairs, golden["pairs"])


def test_all_338_classes_come_back_through_th_tag_rotamers(gpu):
    rng = np.random.default_rng(338)
    classes = np.arange(rr.N_CLASSES)
    types, chi = sidechains.class_centres(classes)
    backbone = np.array([sr.random_backbone(rng, rng.uniform(-30.0, 30.0, 3)) for _ in classes])
    got = sidechains.build_arrays(backbone, types, chi, struct_offsets=np.arange(rr.N_CLASSES + 1), device=gpu)
    table = sidechains.sidechain_table()
    assert got.n_built.tolist() == [len(table[t].atoms) for t in types]
    residues = [(rr.RESIDUES[t], [("N", backbone[r, 0]), ("CA", backbone[r, 1])] + [(nm, got.xyz[r, j]) for j, nm in enumerate(table[t].atoms)])
                for r, t in enumerate(types)]
    cls, back = structure.rotamer_classes(*rr.flatten(residues), device=gpu)
    worst = float(np.nanmax(np.abs((back - chi + 180.0) % 360.0 - 180.0)))
    print(f"338 classes: {int((cls != classes).sum())} differ, worst chi deviation from 60 / 180 / -60: {worst:.3e} degrees")
    assert same_bytes(cls, classes.astype(np.int16))
    assert np.array_equal(np.isnan(back), np.isnan(chi)) and worst < 1e-6


def test_synthetic_residues_of_all_types_equal_the_restatement(gpu, synthetic):
    residues, want, n_built, exact = synthetic
    assert {r[0] for r in residues} == set(rr.RESIDUES) and len(residues) == 200
    assert (np.abs(np.abs(np.array([r[2] for r in residues])) - 180.0) > 1e-6).all()
    backbone, types, chi = arrays(residues)
    got = sidechains.build_arrays(backbone, types, chi, clashes=False, device=gpu)
    assert got.clashes is None and got.pairs is None and got.n_matched is None
    assert same_bytes(got.n_built, n_built) and (n_built > 0).sum() == 190
    check_xyz("synthetic", got.xyz, want, exact)
    worst_len = worst_ang = 0.0
    for r, (res, bb, _) in enumerate(residues):
        at = {"N": bb[0], "CA": bb[1], "C": bb[2]}
        for j, (name, (a, b, c), k, length, angle, off) in enumerate(sr.TREE[res]):
            at[name] = got.xyz[r, j]
            u, v = at[b] - at[c], at[name] - at[c]
            worst_len = max(worst_len, abs(np.linalg.norm(v) - length))
            worst_ang = max(worst_ang, abs(np.degrees(np.arccos(u @ v / np.linalg.norm(u) / np.linalg.norm(v))) - angle))
    print(f"synthetic: worst bond length off the table {worst_len:.3e} Angstrom, worst bond angle {worst_ang:.3e} degrees")
    assert worst_len < 1e-9 and worst_ang < 1e-9


def test_unbuilt_residues(gpu, lib):
    rng = np.random.default_rng(5)
    good = lambda res: (res, sr.random_backbone(rng), sr.random_chi(rng))          # noqa: E731

    def with_nan(res, atom=None, chi=None):
        name, bb, angles = good(res)
        bb, angles = bb.copy(), angles.copy()
        if atom is not None:
            bb[atom, 1] = np.nan
        if chi is not None:
            angles[chi] = np.nan
        return (name, bb, angles)
    line = ("LEU", np.array([[0.0, 0.0, 0.0], [1.5, 0.0, 0.0], [3.0, 0.0, 0.0], [3.0, 1.2, 0.0]]), sr.random_chi(rng))
    residues = [good("LEU"), ("HOH", sr.random_backbone(rng), sr.random_chi(rng)), good("ARG"), good("GLY"), good("TRP"), with_nan("LYS", atom=0),
                good("PHE"), with_nan("SER", atom=2), with_nan("ARG", chi=3), good("MET"), with_nan("SER", chi=1), with_nan("ALA", chi=0),
                with_nan("VAL", chi=3), line, good("TYR"), with_nan("ILE", atom=3), with_nan("GLU", chi=0)]
    built = [True, False, True, False, True, False, True, False, False, True, True, True, True, False, True, True, False]
    want, n_built = sr.restate_build(residues)
    assert ((n_built > 0) == np.array(built)).all()
    backbone, types, chi = arrays(residues)
    assert types[1] == -1
    got = sidechains.build_arrays(backbone, types, chi, device=gpu)                # returns: TH_OK
    assert same_bytes(got.n_built, n_built) and np.array_equal(np.isnan(got.xyz), np.isnan(want))
    assert np.isnan(got.xyz[~np.array(built)]).all() and (got.n_built[~np.array(built)] == 0).all()
    assert (got.clashes[~np.array(built)] == 0).all()
    alone = [sidechains.build_arrays(backbone[r:r + 1], types[r:r + 1], chi[r:r + 1], device=gpu) for r in np.flatnonzero(built)]
    for r, one in zip(np.flatnonzero(built), alone):                               # the neighbours of an unbuilt residue: the same bytes as alone
        assert same_bytes(one.xyz[0], got.xyz[r]) and one.n_built[0] == got.n_built[r], r
    # n_res == 0, only empty structures
    none = sidechains.build_arrays(np.zeros((0, 3, 3)), [], np.zeros((0, 4)), struct_offsets=[0, 0, 0], device=gpu)
    assert none.xyz.shape == (0, 10, 3) and none.pairs.tolist() == [0, 0]
    assert sidechains.build([], device=gpu) == []
    (empty,) = sidechains.build([pdbio.Model(1, [])], device=gpu)
    assert empty.xyz.shape == (0, 10, 3) and empty.pairs == 0 and empty.residues == []


def _clash_case(residues, chain_id, offsets, gpu, distance=sr.CLASH_DISTANCE):
    xyz, _ = sr.restate_build(residues)
    clashes, pairs, margin = sr.restate_clashes(residues, xyz, chain_id, offsets, distance)
    assert margin > 1e-9, margin                           # no distance of the data sits on the threshold
    backbone, types, chi = arrays(residues)
    got = sidechains.build_arrays(backbone, types, chi, struct_offsets=offsets, chain_id=chain_id, clash_distance=distance, device=gpu)
    return got, clashes, pairs, xyz


def test_clash_counts_equal_the_restatement_as_bytes(gpu):
    rng = np.random.default_rng(17)
    sizes = [1, 17, 33, 19, 37, 0, 2]                      # 16-residue workgroups crossed; 19 x 14 = 266 and 37 x 14 = 518 slots: over one and two tiles
    parts = [sr.compact_structure(rng, n) for n in sizes]
    residues = [r for part in parts for r in part]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    chain_id = np.zeros(len(residues), np.int32)
    got, clashes, pairs, _ = _clash_case(residues, chain_id, offsets, gpu)
    print("clashing pairs per structure", pairs.tolist(), "GPU", got.pairs.tolist(), "residues with a clash", int((clashes > 0).sum()), "of", len(residues))
    assert pairs.max() > 10 and pairs[0] == 0
    assert same_bytes(got.clashes, clashes) and same_bytes(got.pairs, pairs)
    wider, clashes3, pairs3, _ = _clash_case(residues, chain_id, offsets, gpu, distance=3.1)
    assert same_bytes(wider.clashes, clashes3) and same_bytes(wider.pairs, pairs3) and pairs3.sum() > pairs.sum()


def _beside(residue, shift):
    res, bb, chi = residue
    return (res, bb + np.asarray(shift), chi)


def test_clash_rules_neighbours_chain_breaks_and_disulfides(gpu):
    rng = np.random.default_rng(29)
    first = ("LEU", sr.random_backbone(rng), sr.random_chi(rng))
    cb = sr.build_residue(*first)["CB"]
    second = ("LEU", sr.random_backbone(rng), sr.random_chi(rng))
    second = _beside(second, np.round(cb - second[1][1] + np.array([0.6, 0.3, 0.2]), 3))       # its CA 0.7 Angstrom from the first's CB
    pair = [first, second]
    offsets = np.array([0, 2], np.int64)
    same, want_same, pairs_same, xyz = _clash_case(pair, np.array([0, 0], np.int32), offsets, gpu)
    split, want_split, pairs_split, _ = _clash_case(pair, np.array([0, 1], np.int32), offsets, gpu)
    apart, want_apart, pairs_apart, _ = _clash_case([first, ("GLY", first[1] + 50.0, first[2]), second], np.zeros(3, np.int32), np.array([0, 3], np.int64), gpu)
    print("chain neighbours", pairs_same.tolist(), "chain break", pairs_split.tolist(), "one residue between", pairs_apart.tolist())
    assert same_bytes(same.clashes, want_same) and same_bytes(same.pairs, pairs_same)
    assert same_bytes(split.clashes, want_split) and same_bytes(split.pairs, pairs_split)
    assert same_bytes(apart.clashes, want_apart) and same_bytes(apart.pairs, pairs_apart)
    # by hand: all (side-chain atom, atom of the other residue) pairs, and those with a side-chain atom at both ends
    atoms = [[(False, p) for p in r[1]] + [(True, p) for p in xyz[k, :4]] for k, r in enumerate(pair)]
    close = [(a, b) for a, pa in atoms[0] for b, pb in atoms[1] if (a or b) and np.linalg.norm(pa - pb) < sr.CLASH_DISTANCE]
    both = sum(1 for a, b in close if a and b)
    assert len(close) > both > 0
    assert pairs_split[0] == pairs_apart[0] == len(close) and pairs_same[0] == both        # a chain break is counted in full
    # SG-SG is skipped, OG-OG at the same place is not
    cys = ("CYS", first[1], np.array([-60.0, 0.0, 0.0, 0.0]))
    for res in ("CYS", "SER"):
        two = [(res, cys[1], cys[2]), _beside((res, cys[1], cys[2]), [0.9, 0.8, -0.7])]
        got, want, pairs, xyz2 = _clash_case(two, np.array([0, 1], np.int32), offsets, gpu)
        atoms = [[(False, "bb", p) for p in r[1]] + [(True, n, p) for n, p in zip(("CB", "G"), xyz2[k, :2])] for k, r in enumerate(two)]
        close = [(na, nb) for a, na, pa in atoms[0] for b, nb, pb in atoms[1] if (a or b) and np.linalg.norm(pa - pb) < sr.CLASH_DISTANCE]
        assert ("G", "G") in close
        print(res, "pairs within the distance", len(close), "counted", pairs.tolist())
        assert same_bytes(got.clashes, want) and same_bytes(got.pairs, pairs)
        assert pairs[0] == len(close) - (1 if res == "CYS" else 0)


def _subset(model, lo, hi):
    return pdbio.Model(1, [r for r in model.residues if not r.hetero][lo:hi])


def test_batches_cut_by_a_tiny_budget_and_two_calls_give_the_same_bytes(gpu, golden):
    ubq_model = pdbio.read_pdb(rr.UBQ)[0]
    structures = [ubq_model, _subset(ubq_model, 0, 31), pdbio.Model(1, []), _subset(ubq_model, 40, 41), ubq_model, _subset(ubq_model, 20, 76)]
    fields = ("xyz", "n_built", "n_matched", "sum_sq", "clashes", "chi")
    for mode in ("native", "class_centres"):
        stats = {}
        whole = sidechains.build(structures, chi=mode, device=gpu, stats=stats)
        assert stats["submissions"] == 1
        budget = 80 * sidechains._RES_BYTES
        runs = sidechains.cut_batches([len(b.residues) for b in whole], budget)
        assert len(runs) >= 4
        stats = {}
        split = sidechains.build(structures, chi=mode, device=gpu, budget_bytes=budget, stats=stats)
        assert stats["submissions"] == len(runs)
        again = sidechains.build(structures, chi=mode, device=gpu)
        alone = [sidechains.build([s], chi=mode, device=gpu)[0] for s in structures]
        for a, b, c, d in zip(whole, split, again, alone):
            for f in fields:
                assert same_bytes(getattr(a, f), getattr(b, f)) and same_bytes(getattr(a, f), getattr(c, f)) and same_bytes(getattr(a, f), getattr(d, f)), f
            assert a.pairs == b.pairs == c.pairs == d.pairs
        assert same_bytes(whole[0].xyz, whole[4].xyz)
        print(mode, "1ubq RMSD", round(whole[0].overall_rmsd, 4), "clashing pairs", whole[0].pairs)
        if mode == "native":
            assert same_bytes(whole[0].n_matched, golden["n_matched"]) and whole[0].overall_rmsd <= RMSD_BOUND
        else:
            assert whole[0].overall_rmsd > golden["rmsd"]              # the bin centres cost something


def test_abi_errors_return_einval_and_launch_nothing(gpu, lib):
    for what, change in BAD_CALLS.items():
        rc, untouched = _call(lib, **change)
        assert rc == _lib.TH_EINVAL and b"th_build_sidechains" in lib.th_last_error() and untouched, what
    rc, untouched = _call(lib)
    assert rc == _lib.TH_OK and not untouched


def test_build_sidechains_cli_end_to_end(gpu, tmp_path, capsys):
    import build_sidechains
    truth = np.load(rr.GOLDEN)["cls"]
    root = tmp_path / "pdb"
    (root / "ub").mkdir(parents=True)
    shutil.copy(rr.UBQ, root / "ub" / "1ubq.pdb1.gz")
    residues = [r for r in pdbio.read_pdb(rr.UBQ)[0].residues if not r.hetero]
    rows = [f"1ubq,A,{r.number},X" for r in residues]
    rows.insert(40, "1ubq,A,999,X")                                     # a row for a residue the file lacks
    probs = np.zeros((77, 338))
    probs[np.delete(np.arange(77), 40), truth] = 1.0
    probs[40, 7] = 1.0
    np.savetxt(tmp_path / "M_rot.csv", probs, delimiter=",", fmt="%g")
    (tmp_path / "map.txt").write_text("\n".join(rows) + "\n")
    out = tmp_path / "out"
    built = build_sidechains.main(build_sidechains.build_parser().parse_args(
        ["--path_to_pdb", str(root), "--path_to_output", str(out), "--path_to_pred_matrix", str(tmp_path / "M_rot.csv"),
         "--path_to_datasetmap", str(tmp_path / "map.txt"), "--device", str(gpu)]))
    said = capsys.readouterr().out
    assert "1 unmatched rows" in said and "in 1 GPU submission(s)" in said
    (tagged,) = structure.tag_rotamers([out / "1ubq_M_rot.pdb"], device=gpu)
    assert same_bytes(tagged.cls, truth) and [r.name for r in tagged.residues] == [r.name for r in residues]
    (model,) = pdbio.read_pdb(out / "1ubq_M_rot.pdb")
    assert sum(len(r.atoms) for r in model.residues) == 4 * 76 + int(built[0].n_built.sum()) and int(built[0].n_built.sum()) == 297
    with open(out / "structure_sidechains.csv", newline="") as f:
        srows = list(csv.reader(f))
    with open(out / "residue_sidechains.csv", newline="") as f:
        rrows = list(csv.reader(f))
    assert srows[0] == build_sidechains.STRUCTURE_COLUMNS and rrows[0] == build_sidechains.RESIDUE_COLUMNS
    assert srows[1][:5] == ["ub/1ubq.pdb1.gz", "76", "70", "70", "297"] and srows[1][7] == "1" and 0.0 < float(srows[1][5]) < 1.5
    assert len(rrows) == 77 and rrows[1][:6] == ["ub/1ubq.pdb1.gz", "A", "1", "MET", "MET", str(int(truth[0]))]
    assert rrows[1][6:10] == ["60.0", "180.0", "180.0", ""] and rrows[1][10:12] == ["4", "4"]
    # without a matrix: the native angles, which leave the error of the table alone
    build_sidechains.main(build_sidechains.build_parser().parse_args(
        ["--path_to_pdb", str(root), "--path_to_output", str(out), "--chi", "native", "--device", str(gpu)]))
    with open(out / "structure_sidechains.csv", newline="") as f:
        native = list(csv.reader(f))
    assert (out / "1ubq_native_chi.pdb").exists() and float(native[1][5]) <= RMSD_BOUND and float(native[1][5]) < float(srows[1][5]) and native[1][7] == "0"
