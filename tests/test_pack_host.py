"""th_pack_sidechains without a GPU: the fixture regenerates from the restatement; the restatement's own bookkeeping (the energy
falls with every move, the final energy equals the energy recomputed from scratch from the final classes, the search converges);
a prior that admits the native class alone leaves the native classes in place; prior_costs on its edge rows; the command-line
parsers; argument errors, which are found before any device is touched; and the CONDITION under which the GPU tests may ask for
equal bytes: for every input tests/test_gpu_pack.py packs, no distance the restatement evaluates lies within 1e-9 Angstrom of a
ladder level."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import pack_restatement as pr  # noqa: E402
import rotamer_restatement as rr  # noqa: E402
import sidechain_restatement as sr  # noqa: E402
from timed_hip import _lib, packer  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return np.load(pr.GOLDEN)


@pytest.fixture(scope="module")
def cases():
    return pr.fixture_cases()


@pytest.fixture(scope="module")
def results(cases):
    return {name: pr.restate_pack(res, chain, prior=prior, **kw) for name, (res, chain, prior, kw) in cases.items()}


def test_the_fixture_regenerates_to_the_same_bytes(golden, capsys):
    import make_pack_golden
    again = make_pack_golden.compute()
    capsys.readouterr()
    assert sorted(again) == sorted(golden.files)
    for key in golden.files:
        a, b = np.asarray(again[key]), golden[key]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), key
    assert str(golden["sha256"]) == pr.ubq_structure()[2]


def test_energy_falls_with_every_move_and_ends_where_a_recount_puts_it(cases, results, golden):
    for name, got in results.items():
        residues, chain, prior, kw = cases[name]
        trace = got["energies"]
        print(name, "energy", trace[0], "->", trace[-1], "moves", got["n_moves"], "sweeps", got["n_sweeps"], "margin", got["margin"])
        assert len(trace) == got["n_moves"] + 1 and all(b < a for a, b in zip(trace, trace[1:])), name
        assert got["energy_initial"] == trace[0] and got["energy_final"] == trace[-1]
        recount = pr.energy_from_scratch(residues, got["cls"], chain, kw.get("ladder", pr.LADDER), kw.get("weight", pr.WEIGHT), prior)
        assert recount == got["energy_final"], name
        assert got["converged"] == 1 and 1 <= got["n_sweeps"] <= pr.MAX_SWEEPS and got["status"] == 0, name
        assert got["energy_final"] == int(golden[name + "_energy"][1]) and got["margin"] > pr.MARGIN_BOUND
        # a residue's cost holds its share of the energy: priors and backbone once, side chain pairs from both ends
        assert (got["cost_final"] >= 0).all() and got["cost_final"].sum() >= got["energy_final"]


@pytest.mark.parametrize("name", ["native", "single_level"])
def test_a_prior_for_the_native_classes_alone_leaves_them_in_place(cases, golden, name):
    residues, chain, _, kw = cases[name]
    _, native_cls, _ = pr.ubq_structure()
    got = pr.restate_pack(residues, chain, prior=pr.native_only_prior(residues, native_cls), **kw)
    packed = np.array([pr.n_candidates(res) > 0 for res, _ in residues]) & (native_cls >= 0)
    assert packed.sum() >= 68 and np.array_equal(got["cls"][packed], native_cls[packed])
    assert pr.chi1_right(residues, got["cls"], native_cls) == (68, 68)
    # and without it: the count the fixture records
    right, total = pr.chi1_right(residues, golden[name + "_cls"], native_cls)
    print(name, "chi1 bins right by sterics alone:", right, "of", total)
    assert [right, total] == golden[name + "_chi1"].tolist() and total == 68


def test_prior_costs_edge_rows(lib):
    matrix = np.zeros((6, rr.N_CLASSES))
    types = [sr.type_index(r) for r in ("SER", "SER", "SER", "GLY", "ALA", "LYS")]
    base = rr.CLASS_BASE["SER"]
    matrix[0, base:base + 3] = [0.5, 0.25, 0.0]                    # a zero: the cap; the rest renormalised over the type: 2/3, 1/3
    matrix[0, 0] = 0.25                                            # mass on another type's class does not count
    matrix[2, base + 1] = 1e-30                                    # a certainty after renormalisation
    matrix[3, rr.CLASS_BASE["GLY"]] = 1.0
    matrix[4, rr.CLASS_BASE["ALA"]] = 0.125
    matrix[5, rr.CLASS_BASE["LYS"]:rr.CLASS_BASE["LYS"] + 81] = 1.0
    matrix[5, rr.CLASS_BASE["LYS"] + 80] = 1e-320                 # so small that -1000 log2 passes the cap
    cost = packer.prior_costs(matrix, types)
    assert cost.dtype == np.int32 and cost.shape == (6, 81)
    assert cost[0, :3].tolist() == [round(-1000 * np.log2(2 / 3)), round(-1000 * np.log2(1 / 3)), 10 ** 6] == [585, 1585, 10 ** 6]
    assert (cost[0, 3:] == 0).all() and (cost[1] == 0).all()                      # an all-zero type sum: no preference
    assert cost[2, :3].tolist() == [10 ** 6, 0, 10 ** 6]
    assert (cost[3] == 0).all() and (cost[4] == 0).all()
    assert cost[5, 80] == 10 ** 6 and (cost[5, :80] == round(1000 * np.log2(80))).all()
    assert packer.prior_costs(np.zeros((1, rr.N_CLASSES)), [-1]).tolist() == [[0] * 81]
    for bad in (np.full((1, rr.N_CLASSES), -0.1), np.full((1, rr.N_CLASSES), np.nan), np.zeros((1, 20)), np.zeros((2, rr.N_CLASSES))):
        with pytest.raises(ValueError):
            packer.prior_costs(bad, [0])
    with pytest.raises(ValueError):
        packer.prior_costs(np.zeros((1, rr.N_CLASSES)), [20])
    assert packer.candidate_counts([0, 5, 8, 14, -1, 15]).tolist() == [1, 0, 81, 81, 0, 3]


def test_every_gpu_input_keeps_its_distances_off_the_ladder():
    """the condition of tests/test_gpu_pack.py, not a measurement: a seeded input that misses it gets another seed"""
    for name, (structures, kw) in pr.gpu_cases().items():
        _, margin = pr.restate_batch(structures, **kw)
        print(f"{name}: margin {margin:.3e}")
        assert margin > pr.MARGIN_BOUND, name


def test_cli_parsers():
    import analyse_rotamers
    import pack_sidechains
    args = pack_sidechains.build_parser().parse_args(["--path_to_pdb", "a", "b", "--path_to_output", "out"])
    assert args.path_to_pdb == ["a", "b"] and args.sequence == "native" and args.prior is None and args.path_to_pred_matrix is None
    assert tuple(args.ladder) == packer.LADDER and args.clash_weight == packer.CLASH_WEIGHT == 2000 and args.max_sweeps == 10
    assert args.clash_distance == 2.5 and args.device == 0
    args = pack_sidechains.build_parser().parse_args(
        ["--path_to_pdb", "a", "--path_to_output", "out", "--path_to_pred_matrix", "m.csv", "--path_to_datasetmap", "map.txt", "--sequence", "predicted",
         "--prior", "none", "--ladder", "2.5", "3", "--clash_weight", "7", "--max_sweeps", "0", "--clash_distance", "3.0"])
    assert args.sequence == "predicted" and args.prior == "none" and args.ladder == [2.5, 3.0] and args.clash_weight == 7 and args.max_sweeps == 0
    with pytest.raises(SystemExit):
        pack_sidechains.build_parser().parse_args(["--path_to_pdb", "a", "--sequence", "scwrl"])
    args = analyse_rotamers.build_parser().parse_args(["--path_to_pred_matrix", "m.csv"])
    assert not hasattr(args, "pack")                               # the reference's namespace is left as it is
    args = analyse_rotamers.build_parser().parse_args(["--path_to_pred_matrix", "m.csv", "--pack", "--path_to_pdb", "pdb"])
    assert args.pack is True
    with pytest.raises(SystemExit):                                 # --pack packs structures: it needs them
        analyse_rotamers.main(analyse_rotamers.build_parser().parse_args(
            ["--path_to_pred_matrix", "m.csv", "--pack", "--path_to_rotamer_labels", "labels.json"]))


def _call(lib, **change):
    """th_pack_sidechains on three residues in two structures with one argument changed; the outputs must stay untouched"""
    kw = dict(backbone=np.zeros((3, 3, 3)), types=np.array([0, 1, 2], np.int8), chain=None, offsets=np.array([0, 2, 3], np.int64), n_struct=2,
              n_res=3, ladder=np.array([2.0, 2.5]), n_levels=2, prior=None, weight=2000, max_sweeps=10, flags=0, cls=np.full(3, 77, np.int16),
              cost0=np.full(3, 77, np.int64), cost1=np.full(3, 77, np.int64), e0=np.full(2, 77, np.int64), e1=np.full(2, 77, np.int64),
              search=np.full((2, 4), 77, np.int32))
    kw.update(change)
    p = _lib.ptr
    rc = lib.th_pack_sidechains(0, p(kw["backbone"]), p(kw["types"]), p(kw["chain"]), p(kw["offsets"]), kw["n_struct"], kw["n_res"], p(kw["ladder"]),
                                kw["n_levels"], p(kw["prior"]), kw["weight"], kw["max_sweeps"], kw["flags"], p(kw["cls"]), p(kw["cost0"]), p(kw["cost1"]),
                                p(kw["e0"]), p(kw["e1"]), p(kw["search"]), None)
    untouched = all((kw[k] == 77).all() for k in ("cls", "cost0", "cost1", "e0", "e1", "search") if kw[k] is not None)
    return rc, untouched


def _prior(value, at=(1, 2)):
    prior = np.zeros((3, 81), np.int32)
    prior[at] = value
    return prior


BAD_CALLS = {
    "negative n_res": dict(n_res=-1),
    "negative n_struct": dict(n_struct=-1),
    "too many residues": dict(n_res=2 ** 24 + 1),
    "offsets do not end at n_res": dict(n_res=2),
    "offsets do not start at 0": dict(offsets=np.array([1, 2, 3], np.int64)),
    "offsets decrease": dict(offsets=np.array([0, 4, 3], np.int64)),
    "offsets NULL": dict(offsets=None),
    "type 20": dict(types=np.array([0, 20, 2], np.int8)),
    "type -2": dict(types=np.array([-2, 1, 2], np.int8)),
    "backbone NULL": dict(backbone=None),
    "res_type NULL": dict(types=None),
    "ladder NULL": dict(ladder=None),
    "no level": dict(n_levels=0),
    "nine levels": dict(ladder=np.arange(1.0, 10.0), n_levels=9),
    "ladder not increasing": dict(ladder=np.array([2.5, 2.5])),
    "ladder decreasing": dict(ladder=np.array([2.5, 2.0])),
    "ladder level 0": dict(ladder=np.array([0.0, 2.0])),
    "ladder level NaN": dict(ladder=np.array([2.0, np.nan])),
    "ladder level infinite": dict(ladder=np.array([2.0, np.inf])),
    "weight 0": dict(weight=0),
    "weight above the cap": dict(weight=10 ** 6 + 1),
    "negative max_sweeps": dict(max_sweeps=-1),
    "max_sweeps 1001": dict(max_sweeps=1001),
    "negative prior": dict(prior=_prior(-1)),
    "prior above the cap": dict(prior=_prior(10 ** 6 + 1)),
    "unknown flag": dict(flags=2),
    "out_cls NULL": dict(cls=None),
    "out_cost_initial NULL": dict(cost0=None),
    "out_cost_final NULL": dict(cost1=None),
    "out_energy_initial NULL": dict(e0=None),
    "out_energy_final NULL": dict(e1=None),
    "out_search NULL": dict(search=None),
    "n_struct 0 with residues": dict(n_struct=0),
}


@pytest.mark.parametrize("what", list(BAD_CALLS))
def test_abi_errors_are_found_before_any_device_is_touched(lib, what):
    rc, untouched = _call(lib, **BAD_CALLS[what])
    assert rc == _lib.TH_EINVAL and b"th_pack_sidechains" in lib.th_last_error() and untouched, what


def test_empty_call_and_python_argument_errors(lib):
    assert lib.th_pack_sidechains(0, None, None, None, None, 0, 0, _lib.ptr(np.array([2.5])), 1, None, 1, 0, 0, None, None, None, None, None, None,
                                  None) == _lib.TH_OK
    with pytest.raises(ValueError):
        packer.pack_arrays(np.zeros((3, 2, 3)), [0, 1, 2])
    with pytest.raises(ValueError):
        packer.pack_arrays(np.zeros((3, 3, 3)), [0, 1, 2], chain_id=[0, 0])
    with pytest.raises(ValueError):
        packer.pack_arrays(np.zeros((3, 3, 3)), [0, 1, 2], prior_cost=np.zeros((3, 27), np.int32))
    with pytest.raises(_lib.TimedHipError) as err:
        packer.pack_arrays(np.zeros((3, 3, 3)), [0, 1, 2], ladder=(2.5, 2.0))
    assert err.value.code == _lib.TH_EINVAL
    with pytest.raises(ValueError):
        packer.pack([], sequence="scwrl")
    with pytest.raises(ValueError):
        packer.pack([], sequence="predicted")
    with pytest.raises(ValueError):
        packer.pack([], prior="matrix")
    assert packer.cut_batches([100, 100, 100], 150 * packer._UNIT_BYTES) == [(0, 1), (1, 2), (2, 3)]
    assert packer.cut_batches([100, 100, 100]) == [(0, 3)]
