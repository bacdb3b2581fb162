"""th_pack_sidechains on the GPU against the NumPy restatement (tests/pack_restatement.py) and the committed fixture of 1ubq.
Every output must equal the restatement's as BYTES: what the search decides is an integer once no distance of the input lies
within 1e-9 Angstrom of a ladder level (tests/test_pack_host.py checks that condition for every input used here, without a GPU),
and float64 placement differences of about 1e-15 Angstrom cannot cross 1e-9.

Also: the energy against the clash count of th_build_sidechains, a kernel that already exists; a ragged batch against every
structure alone and against the batch reversed; more structures than a small grid; the neighbour and disulfide rules; max_sweeps 0
and 1; a structure over the per-structure limit; ABI errors; pack_sidechains.py and analyse_rotamers.py --pack end to end.

Each test prints its figures before it asserts."""
import csv
import json
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pack_restatement as pr  # noqa: E402
import rotamer_restatement as rr  # noqa: E402
from test_pack_host import BAD_CALLS, _call, _prior  # noqa: E402
from timed_hip import _lib, packer, pdbio, sidechains, structure  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return np.load(pr.GOLDEN)


@pytest.fixture(scope="module")
def cases():
    return pr.gpu_cases()


def same_bytes(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def run(structures, gpu, ladder=pr.LADDER, weight=pr.WEIGHT, max_sweeps=pr.MAX_SWEEPS):
    backbone, types, offsets, chain, prior = pr.flat(structures)
    return packer.pack_arrays(backbone, types, offsets, chain, prior, ladder, weight, max_sweeps, device=gpu)


def check(what, got, want):
    for f in pr.FIELDS:
        assert same_bytes(getattr(got, f), want[f]), (what, f, getattr(got, f), want[f])


def against_the_restatement(what, structures, kw, gpu):
    want, margin = pr.restate_batch(structures, **kw)
    got = run(structures, gpu, **kw)
    print(f"{what}: {len(structures)} structure(s), energy {want['energy_initial'].tolist()[:6]} -> {want['energy_final'].tolist()[:6]}, "
          f"sweeps {want['n_sweeps'].tolist()[:6]}, moves {want['n_moves'].tolist()[:6]}; GPU energy {got.energy_final.tolist()[:6]}; margin {margin:.2e}")
    assert margin > pr.MARGIN_BOUND
    check(what, got, want)
    return got, want


@pytest.mark.parametrize("name", ["native", "prior", "predicted", "single_level"])
def test_fixture_cases_equal_the_fixture_as_bytes(gpu, golden, cases, name):
    structures, kw = cases["fixture_" + name]
    assert str(golden["sha256"]) == pr.ubq_structure()[2]
    if structures[0][2] is not None:
        assert same_bytes(np.asarray(structures[0][2], np.int32), golden[name + "_prior"])
    got = run(structures, gpu, **kw)
    print(f"{name}: energy {int(got.energy_initial[0])} -> {int(got.energy_final[0])} in {int(got.n_sweeps[0])} sweeps, {int(got.n_moves[0])} moves; "
          f"fixture {golden[name + '_energy'].tolist()} {golden[name + '_search'].tolist()}")
    assert same_bytes(got.cls, golden[name + "_cls"])
    assert same_bytes(got.cost_initial, golden[name + "_cost_initial"]) and same_bytes(got.cost_final, golden[name + "_cost_final"])
    assert [int(got.energy_initial[0]), int(got.energy_final[0])] == golden[name + "_energy"].tolist()
    assert [int(got.n_sweeps[0]), int(got.n_moves[0]), int(got.converged[0]), int(got.status[0])] == golden[name + "_search"].tolist()
    assert got.converged[0] == 1 and got.energy_final[0] < got.energy_initial[0]


@pytest.mark.parametrize("name", ["cross_ubq", "cross_compact"])
def test_energy_equals_the_clash_count_of_th_build_sidechains(gpu, cases, name):
    """ladder (clash_distance), weight 1, no prior: the energy IS the number of clashing pairs of the chosen classes"""
    structures, kw = cases[name]
    assert kw == dict(ladder=(sidechains.CLASH_DISTANCE,), weight=1)
    got, _ = against_the_restatement(name, structures, kw, gpu)
    backbone, types, offsets, chain, _ = pr.flat(structures)
    built_types, chi = sidechains.class_centres(got.cls)
    assert (built_types[got.cls >= 0] == types[got.cls >= 0]).all()
    built = sidechains.build_arrays(backbone, built_types, chi, offsets, chain, clash_distance=sidechains.CLASH_DISTANCE, device=gpu)
    first = np.where(got.cls >= 0, [rr.CLASS_BASE.get(r[0], 0) for r in structures[0][0]], -1)
    before = sidechains.build_arrays(backbone, *sidechains.class_centres(first), offsets, chain, device=gpu)
    print(f"{name}: energy {int(got.energy_final[0])}, clashing pairs of the packed classes {int(built.pairs[0])}, of the first class everywhere {int(before.pairs[0])}")
    assert int(got.energy_final[0]) == int(built.pairs[0]) < int(before.pairs[0])
    assert same_bytes(got.cost_final, built.clashes.astype(np.int64))               # a residue's cost: the pairs its side chain is in
    if name == "cross_compact":
        assert len(structures[0][0]) == 27 and int(before.pairs[0]) > 100          # it clashes heavily


def test_ragged_batch_alone_and_reversed(gpu, cases):
    structures, kw = cases["ragged"]
    assert [len(s[0]) for s in structures] == pr.RAGGED_SIZES == [1, 2, 0, 19, 37, 76]
    names = [r[0] for s in structures for r in s[0]]
    assert "ARG" in names and "LYS" in names and "HOH" in names and {r[0] for r in structures[1][0]} == {"ALA", "GLY"}
    assert np.isnan(np.array([r[1] for r in structures[4][0]])).any()
    got, want = against_the_restatement("ragged", structures, kw, gpu)
    assert (want["n_moves"] > 0).sum() >= 3 and got.cls[1] == rr.CLASS_BASE["ALA"] and got.cls[2] == -1
    offsets = np.concatenate([[0], np.cumsum(pr.RAGGED_SIZES)])
    back = run(structures[::-1], gpu, **kw)
    back_offsets = np.concatenate([[0], np.cumsum(pr.RAGGED_SIZES[::-1])])
    again = run(structures, gpu, **kw)
    for s in range(len(structures)):
        alone = run([structures[s]], gpu, **kw)
        t = len(structures) - 1 - s
        for f in ("cls", "cost_initial", "cost_final"):
            mine = getattr(got, f)[offsets[s]:offsets[s + 1]]
            assert same_bytes(mine, getattr(alone, f)) and same_bytes(mine, getattr(back, f)[back_offsets[t]:back_offsets[t + 1]]), (s, f)
        for f in ("energy_initial", "energy_final", "n_sweeps", "n_moves", "converged", "status"):
            assert getattr(got, f)[s] == getattr(alone, f)[0] == getattr(back, f)[t], (s, f)
    for f in pr.FIELDS:
        assert same_bytes(getattr(got, f), getattr(again, f)), f                   # two calls give the same bytes


def test_more_structures_than_a_small_grid(gpu, cases):
    structures, kw = cases["many_small"]
    assert len(structures) == 70 and {len(s[0]) for s in structures} == {1, 2}
    got, want = against_the_restatement("many_small", structures, kw, gpu)
    assert (got.status == 0).all() and (got.converged == 1).all()


def test_a_structure_longer_than_the_lds_tile_is_streamed(gpu, cases):
    structures, kw = cases["streamed"]
    assert [len(s[0]) for s in structures] == [203, 5]                             # 203 > 200 residues: two tiles
    got, want = against_the_restatement("streamed", structures, kw, gpu)
    assert want["n_moves"][0] > 0 and want["n_sweeps"][0] >= 2
    alone = run([structures[1]], gpu, **kw)                                        # resident when alone, resident beside a streamed one
    assert same_bytes(got.cls[203:], alone.cls) and got.energy_final[1] == alone.energy_final[0]


def test_neighbours_chain_breaks_and_disulfides(gpu, cases):
    got = {}
    for name in ("neighbours", "chain_break", "CYS", "SER"):
        structures, kw = cases["rule_" + name]
        kw = dict(kw, max_sweeps=0)                                                # the initial state: the backbone penalties alone decide
        got[name], _ = against_the_restatement(name, structures, kw, gpu)
        full, _ = against_the_restatement(name + ", searched", structures, cases["rule_" + name][1], gpu)
        assert full.energy_final[0] <= got[name].energy_final[0]
    # the second residue's backbone sits on the first one's CB: counted in full across a chain break, not at all between neighbours
    print("initial energies: neighbours", int(got["neighbours"].energy_initial[0]), "chain break", int(got["chain_break"].energy_initial[0]))
    assert got["chain_break"].energy_initial[0] > got["neighbours"].energy_initial[0]
    # by hand, a third way: every pair of atoms across the two residues (they are of different chains, so all count) with a side
    # chain atom in it, without the SG-SG pair for CYS and with the OG-OG pair for SER
    for res, gamma in (("CYS", "SG"), ("SER", "OG")):
        (residues, chain, _), = cases["rule_" + res][0]
        k = [int(c) - rr.CLASS_BASE[res] for c in got[res].cls]
        side = [pr.candidates_of(r, bb)[q] for (r, bb), q in zip(residues, k)]
        atoms = [[("bb", p) for p in bb] + list(side[i].items()) for i, (_, bb) in enumerate(residues)]
        levels = lambda p, q: int((np.linalg.norm(p - q) < np.array(pr.LADDER)).sum())       # noqa: E731
        total = sum(levels(p, q) for a, p in atoms[0] for b, q in atoms[1] if (a != "bb" or b != "bb") and not (a == b == "SG"))
        gammas = levels(side[0][gamma], side[1][gamma])
        print(f"{res}: {gamma}-{gamma} under {gammas} levels; by hand {total} levels, GPU energy {int(got[res].energy_initial[0])}")
        assert gammas > 0 and pr.WEIGHT * total == int(got[res].energy_initial[0])


def test_max_sweeps_0_and_1(gpu, cases):
    zero, want0 = against_the_restatement("max_sweeps 0", *cases["sweeps_0"], gpu)
    one, want1 = against_the_restatement("max_sweeps 1", *cases["sweeps_1"], gpu)
    assert zero.n_sweeps[0] == 0 and zero.n_moves[0] == 0 and zero.converged[0] == 0
    assert same_bytes(zero.cost_initial, zero.cost_final) and zero.energy_initial[0] == zero.energy_final[0]
    assert one.n_sweeps[0] == 1 and one.n_moves[0] > 0 and one.converged[0] == 0 and one.energy_final[0] < zero.energy_final[0]
    assert same_bytes(one.cost_initial, zero.cost_initial)
    # nothing could move: ALA and GLY alone
    for sweeps in (0, 5):
        got, _ = against_the_restatement(f"nothing to move, max_sweeps {sweeps}", cases["still"][0], dict(max_sweeps=sweeps), gpu)
        assert got.converged[0] == 1 and got.n_sweeps[0] == 0 and got.cls.tolist() == [rr.CLASS_BASE["ALA"], -1]


def test_a_structure_over_the_limit_carries_its_status(gpu, cases):
    structures, kw = cases["limit"]
    n = packer.MAX_STRUCT_RESIDUES + 1 == pr.MAX_STRUCT + 1 and pr.MAX_STRUCT + 1
    assert [len(s[0]) for s in structures][::2] == [n, n - 1] and n - 1 >= 1024
    got, _ = against_the_restatement("over the limit", structures, kw, gpu)
    alone = run([structures[1]], gpu)
    assert got.status.tolist() == [packer.TH_PACK_TOO_LONG, 0, 0] and got.converged.tolist() == [0, 1, 1]
    assert (got.cls[:n] == -1).all() and (got.cost_final[:n] == 0).all() and got.energy_final[0] == 0
    lo, hi = n, n + len(structures[1][0])
    assert same_bytes(got.cls[lo:hi], alone.cls) and same_bytes(got.cost_final[lo:hi], alone.cost_final) and got.energy_final[1] == alone.energy_final[0]
    assert alone.energy_final[0] < alone.energy_initial[0] and (got.cls[hi:] == -1).all()


def test_abi_errors_return_einval_and_launch_nothing(gpu, lib):
    for what, change in BAD_CALLS.items():
        rc, untouched = _call(lib, **change)
        assert rc == _lib.TH_EINVAL and b"th_pack_sidechains" in lib.th_last_error() and untouched, what
    rc, untouched = _call(lib)
    assert rc == _lib.TH_OK and not untouched
    rc, untouched = _call(lib, prior=_prior(-5, at=(1, 3)))                          # CYS has 3 candidates: entry 3 is not read
    assert rc == _lib.TH_OK and not untouched


def _ubq_folder(tmp_path):
    root = tmp_path / "pdb"
    (root / "ub").mkdir(parents=True)
    shutil.copy(rr.UBQ, root / "ub" / "1ubq.pdb1.gz")
    return root


def test_pack_sidechains_cli_end_to_end(gpu, tmp_path, capsys, golden):
    import analyse_rotamers
    import pack_sidechains
    root = _ubq_folder(tmp_path)
    residues = [r for r in pdbio.read_pdb(rr.UBQ)[0].residues if not r.hetero]
    rows = [f"1ubq,A,{r.number},X" for r in residues]
    rows.insert(40, "1ubq,A,999,X")                                     # a row for a residue the file lacks
    rng = np.random.default_rng(pr.PRIOR_SEED)
    probs = rng.dirichlet(np.full(rr.N_CLASSES, 0.3), size=76)          # the matrix of the fixture's case "prior"
    np.savetxt(tmp_path / "M_rot.csv", np.insert(probs, 40, probs[0], axis=0), delimiter=",", fmt="%.17g")
    (tmp_path / "map.txt").write_text("\n".join(rows) + "\n")
    out = tmp_path / "out"
    common = ["--path_to_pdb", str(root), "--path_to_output", str(out), "--device", str(gpu)]
    with_matrix = common + ["--path_to_pred_matrix", str(tmp_path / "M_rot.csv"), "--path_to_datasetmap", str(tmp_path / "map.txt")]
    (packed,) = pack_sidechains.main(pack_sidechains.build_parser().parse_args(with_matrix))
    said = capsys.readouterr().out
    assert "1 unmatched rows" in said and "in 1 GPU submission(s)" in said and "0 not converged" in said
    # the native sequence under the matrix's prior: the fixture's case, through files
    assert same_bytes(packed.cls, golden["prior_cls"]) and [packed.energy_initial, packed.energy_final] == golden["prior_energy"].tolist()
    assert (out / "1ubq_packed_M_rot.pdb").exists()
    labels = analyse_rotamers.load_rotamer_labels(out / "rotamer_labels.json")
    assert labels == {"1ubqA": [None if c < 0 else int(c) for c in packed.cls.tolist()]}
    (tagged,) = structure.tag_rotamers([out / "1ubq_packed_M_rot.pdb"], device=gpu)
    on = packed.cls >= 0
    assert on.sum() == 70 and same_bytes(tagged.cls[on], packed.cls[on]) and [r.name for r in tagged.residues] == [r.name for r in residues]
    with open(out / "structure_packing.csv", newline="") as f:
        srows = list(csv.reader(f))
    with open(out / "residue_packing.csv", newline="") as f:
        rrows = list(csv.reader(f))
    assert srows[0] == pack_sidechains.STRUCTURE_COLUMNS and rrows[0] == pack_sidechains.RESIDUE_COLUMNS and len(srows) == 2 and len(rrows) == 77
    assert srows[1][:9] == ["ub/1ubq.pdb1.gz", "76", "70", str(packed.energy_initial), str(packed.energy_final)] + [str(v) for v in golden["prior_search"]]
    assert srows[1][9] == "297" and 0.5 < float(srows[1][10]) < 3.4 and srows[1][11] == str(packed.built.pairs) and srows[1][12] == "1"
    assert rrows[1][:6] == ["ub/1ubq.pdb1.gz", "A", "1", "MET", "MET", str(int(packed.cls[0]))] and rrows[1][9] == ""
    assert [int(r[10]) for r in rrows[1:]] == golden["prior_cost_initial"].tolist() and [int(r[11]) for r in rrows[1:]] == golden["prior_cost_final"].tolist()
    # without a matrix: sterics alone, the fixture's case "native"; the predicted sequence of the matrix packs other types
    (plain,) = pack_sidechains.main(pack_sidechains.build_parser().parse_args(common))
    assert same_bytes(plain.cls, golden["native_cls"]) and (out / "1ubq_packed.pdb").exists() and plain.unmatched_rows == 0
    print("sterics alone: RMSD", round(plain.built.overall_rmsd, 3), "clashing pairs", plain.built.pairs, "; with the prior", round(packed.built.overall_rmsd, 3), packed.built.pairs)
    assert plain.built.pairs == int(golden["native_pairs"]) and abs(plain.built.overall_rmsd - float(golden["native_rmsd"])) < 1e-9
    (predicted,) = pack_sidechains.main(pack_sidechains.build_parser().parse_args(with_matrix + ["--sequence", "predicted", "--prior", "none"]))
    want = np.searchsorted([rr.CLASS_BASE[r] for r in rr.RESIDUES], np.argmax(probs, axis=1), side="right") - 1
    assert predicted.res_type.tolist() == want.tolist() and predicted.converged
    (model,) = pdbio.read_pdb(out / "1ubq_packed_M_rot.pdb")
    assert [r.name for r in model.residues] == [rr.RESIDUES[t] for t in want]


def test_analyse_rotamers_pack_end_to_end(gpu, tmp_path, golden):
    import analyse_rotamers
    root = _ubq_folder(tmp_path)
    rng = np.random.default_rng(8)
    probs = rng.dirichlet(np.full(338, 0.05), 76)
    truth = np.load(rr.GOLDEN)["cls"]
    probs[np.arange(0, 76, 2), truth[::2]] += 0.5                     # a model that is right half of the time
    np.savetxt(tmp_path / "M_rot.csv", probs.astype(np.float16), delimiter=",")
    (tmp_path / "map.txt").write_text("ignore_uncommon False\ninclude_pdbs\n##########\n1ubqA 76\n")
    common = ["--path_to_pred_matrix", str(tmp_path / "M_rot.csv"), "--path_to_datasetmap", str(tmp_path / "map.txt"), "--device", str(gpu), "--path_to_pdb", str(root)]
    plain = analyse_rotamers.main(analyse_rotamers.build_parser().parse_args(common + ["--output_path", str(tmp_path / "a")]))
    packed = analyse_rotamers.main(analyse_rotamers.build_parser().parse_args(common + ["--output_path", str(tmp_path / "b"), "--pack"]))
    a, b = tmp_path / "a_M_rot", tmp_path / "b_M_rot"
    assert plain == packed
    before = sorted(p.name for p in a.iterdir())
    assert before == sorted(["rotamer_labels.json", "results_M_rot_vs_original.txt", "results_M_rot_vs_original.json",
                             "cm_M_rot_vs_original_unweighted.csv", "cm_M_rot_vs_original_weighted.csv"])
    for name in before:                                               # without --pack: the same files with the same bytes as with it
        assert (a / name).read_bytes() == (b / name).read_bytes(), name
    new = sorted(set(p.name for p in b.iterdir()) - set(before))
    assert new == sorted(["1ubq_packed_M_rot.pdb", "1ubq_wt_packed.pdb", "packing_scores.csv"] +
                         [f"{stem}_M_rot_vs_{kind}{ext}" for kind in ("packed_M_rot", "wt_packed")
                          for stem, ext in (("results", ".txt"), ("results", ".json"), ("cm", "_unweighted.csv"), ("cm", "_weighted.csv"))])
    # analysis 3 packs the native sequence by sterics alone: the fixture's case "native"
    (tagged,) = structure.tag_rotamers([b / "1ubq_wt_packed.pdb"], device=gpu)
    on = golden["native_cls"] >= 0
    assert same_bytes(tagged.cls[on], golden["native_cls"][on])
    lines = (b / "packing_scores.csv").read_text().splitlines()
    assert lines[0] == "PDB,score_rot,score_real" and len(lines) == 2
    key, score_rot, score_real = lines[1].split(",")
    assert key == "1ubqA" and int(score_real) == int(golden["native_energy"][1]) and int(score_rot) >= 0
    results = json.loads((b / "results_M_rot_vs_wt_packed.json").read_text())
    assert results["n_labelled"] == 76 and 0.0 <= results["accuracy_1"] <= 1.0
