"""th_lddt on the GPU against the NumPy restatement (tests/lddt_restatement.py) and the committed fixture: the five cases on the CA
atoms of 1ubq, the ragged batch of every size at which the tiling changes (the kernel's tile is 256 positions: 255, 256, 257 and 1025
are in it), exact ties, radii that include everything and nothing, custom thresholds, non-finite positions, and lddt() /
analyse_models.py --lddt end to end.

All outputs are integers and must be exact.  That is fair only if no decision sits on an edge, so each test first asserts ON THE
RESTATEMENT that no d_ref lies within 1e-9 Angstrom of the radius and no |d_ref - d_mob| within 1e-9 of a threshold, and that the
float64 and the long double restatement give the same integers.  (The tie case is the exception by construction: its roots are
exact, so both sides of each tie are decided by the strict inequality alone.)  Each test prints N, C and the edge before it asserts;
profiles/lddt.txt records them.
"""
import csv
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lddt_restatement as lr  # noqa: E402
import superpose_restatement as sr  # noqa: E402
from timed_hip import lddt, superpose  # noqa: E402

pytestmark = pytest.mark.gpu

EDGE = 1e-9


@pytest.fixture(scope="module")
def golden():
    return np.load(lr.GOLDEN)


@pytest.fixture(scope="module")
def cases():
    return sr.ubq_cases()


@pytest.fixture(scope="module")
def ragged():
    """the ragged batch flattened and its float64 restatement: computed once, shared, never changed"""
    pairs = sr.ragged_batch()
    ref, mob, offsets = sr.flatten(pairs)
    return pairs, ref, mob, offsets, lr.restate_batch(ref, mob, offsets)


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def conditioned(what, ref, mob, offsets, radius=lr.RADIUS, thresholds=lr.THRESHOLDS, float64=None):
    """the float64 restatement of a batch, after the condition on the inputs: no decision within EDGE of its tie, and the same
    integers in long double"""
    residue, pair, edge = float64 or lr.restate_batch(ref, mob, offsets, radius, thresholds)
    exact = lr.restate_batch(ref, mob, offsets, radius, thresholds, dtype=np.longdouble)
    print(f"{what}: N {int(pair[:, 1].sum())} C {pair[:, 2:].sum(axis=0).tolist()} over {len(pair)} pair(s), edge {edge:.3e}")
    assert edge > EDGE, (what, edge)
    assert same_bytes(residue, exact[0]) and same_bytes(pair, exact[1]), what
    return residue, pair


def test_ubq_cases_equal_the_fixture(gpu, golden, cases):
    assert str(golden["sha256"]) == sr.inputs_sha256(cases)
    ref, mob, offsets = sr.flatten([cases[name] for name in lr.CASES])
    residue, pair = conditioned("1ubq cases", ref, mob, offsets)
    got = lddt.lddt_arrays(ref, mob, offsets, device=gpu)
    assert got.residue.dtype == np.int32 and got.pair.dtype == np.int64
    for k, name in enumerate(lr.CASES):
        rows, totals = got.residue[76 * k:76 * k + 76], got.pair[k]
        print(name, "n_valid, N, C", totals.tolist(), "lddt", lr.score(totals))
        assert same_bytes(rows, golden[f"{name}_residue"]) and same_bytes(totals, golden[f"{name}_pair"]), name
    assert same_bytes(got.residue, residue) and same_bytes(got.pair, pair)
    assert same_bytes(got.residue[3 * 76:4 * 76], got.residue[:76]) and same_bytes(got.pair[3], got.pair[0])       # mirror: the bytes of rigid
    assert lr.score(got.pair[0]) == 1.0 and got.pair[4, 0] == 73 and not got.residue[4 * 76 + np.array([3, 11, 40])].any()


def test_ragged_batch_equals_the_restatement_and_each_pair_alone(gpu, ragged):
    pairs, ref, mob, offsets, float64 = ragged
    sizes = [len(r) for r, _ in pairs]
    assert sorted(set(sizes)) == list(sr.SIZES) and len(pairs) == 39 and sizes != sorted(sizes)
    residue, pair = conditioned("ragged batch", ref, mob, offsets, float64=float64)
    ordered = int((pair[:, 0] * (pair[:, 0] - 1)).sum())
    assert 0 < pair[:, 1].sum() < ordered                                        # included and excluded pairs, both
    got = lddt.lddt_arrays(ref, mob, offsets, device=gpu)
    assert same_bytes(got.residue, residue) and same_bytes(got.pair, pair)
    again = lddt.lddt_arrays(ref, mob, offsets, device=gpu)
    assert same_bytes(again.residue, got.residue) and same_bytes(again.pair, got.pair)           # a second run: the same bytes
    for k, (r, m) in enumerate(pairs):                                          # a pair alone: the same bytes as in the batch
        a, b = int(offsets[k]), int(offsets[k + 1])
        alone = lddt.lddt_arrays(r, m, [0, len(r)], device=gpu)
        assert same_bytes(alone.residue, got.residue[a:b]) and same_bytes(alone.pair[0], got.pair[k]), (k, len(r))
    empty = [k for k, n in enumerate(sizes) if n < 2]
    assert not got.pair[empty, 1:].any() and got.pair[empty, 0].tolist() == [sizes[k] for k in empty]


def test_tie_case_on_the_gpu(gpu):
    pairs, residue, pair = lr.tie_pairs()
    ref, mob, offsets = sr.flatten(pairs)
    for dtype in (np.float64, np.longdouble):
        restated = lr.restate_batch(ref, mob, offsets, dtype=dtype)
        assert restated[2] == 0.0 and same_bytes(restated[0], residue) and same_bytes(restated[1], pair)
    got = lddt.lddt_arrays(ref, mob, offsets, device=gpu)
    print("tie case: N", int(got.pair[:, 1].sum()), "C", got.pair[:, 2:].sum(axis=0).tolist(), "edge 0 (exact roots)")
    assert same_bytes(got.residue, residue) and same_bytes(got.pair, pair)
    inside = lddt.lddt_arrays(ref, mob, offsets, radius=np.nextafter(15.0, 16.0), device=gpu)     # the next radius includes d_ref = 15
    want = lr.restate_batch(ref, mob, offsets, radius=np.nextafter(15.0, 16.0))
    assert inside.residue[:2].tolist() == [[1, 1, 1, 1, 1]] * 2 and same_bytes(inside.residue, want[0]) and same_bytes(inside.pair, want[1])
    limits = [np.nextafter(t, 8.0) for t in lr.THRESHOLDS]                       # the next thresholds preserve the ties
    wider = lddt.lddt_arrays(ref, mob, offsets, thresholds=limits, device=gpu)
    want = lr.restate_batch(ref, mob, offsets, thresholds=limits)
    assert wider.pair[:, 2:].sum() > got.pair[:, 2:].sum() and same_bytes(wider.residue, want[0]) and same_bytes(wider.pair, want[1])


def test_a_radius_that_includes_everything_and_one_that_includes_nothing(gpu, cases, ragged):
    pairs, ref, mob, offsets, _ = ragged
    keep = [[len(r) for r, _ in pairs].index(n) for n in (3, 65, 257)]
    part_ref, part_mob, part_offsets = sr.flatten([pairs[k] for k in keep] + [cases["invalid"]])
    residue, pair = conditioned("radius 1e30", part_ref, part_mob, part_offsets, radius=1e30)
    got = lddt.lddt_arrays(part_ref, part_mob, part_offsets, radius=1e30, device=gpu)
    assert same_bytes(got.residue, residue) and same_bytes(got.pair, pair)
    for k in range(len(keep) + 1):                                              # every valid ordered pair is included
        rows, n_valid = got.residue[part_offsets[k]:part_offsets[k + 1]], int(got.pair[k, 0])
        valid = np.isfinite(part_ref[part_offsets[k]:part_offsets[k + 1]]).all(axis=1) & np.isfinite(part_mob[part_offsets[k]:part_offsets[k + 1]]).all(axis=1)
        assert n_valid == valid.sum() and (rows[valid, 0] == n_valid - 1).all() and not rows[~valid].any()
        assert got.pair[k, 1] == n_valid * (n_valid - 1)
    assert got.pair[-1, 0] == 73
    ref, mob, offsets = sr.flatten([cases["noise"], cases["hinge"]])
    residue, pair = conditioned("radius 1.0 on 1ubq", ref, mob, offsets, radius=1.0)
    got = lddt.lddt_arrays(ref, mob, offsets, radius=1.0, device=gpu)
    assert not got.residue.any() and got.pair.tolist() == [[76, 0, 0, 0, 0, 0]] * 2 and same_bytes(got.residue, residue) and same_bytes(got.pair, pair)
    (nothing,) = lddt.lddt([_layouts(cases["noise"])], radius=1.0, device=gpu)
    assert nothing.error is None and np.isnan(nothing.lddt) and np.isnan(nothing.lddt_i).all() and nothing.n_included == 0 and nothing.n_valid == 76
    assert all(np.isnan(p) for p in nothing.preserved)


def _layouts(pair):
    from timed_hip import pdbio
    residues = [pdbio.Residue("A", str(k + 1), "GLY") for k in range(len(pair[0]))]
    return superpose.AtomLayout(np.asarray(pair[0]), residues), superpose.AtomLayout(np.asarray(pair[1]), residues)


def test_custom_thresholds(gpu, cases):
    limits = (0.25, 0.75, 3.0, 6.0)
    ref, mob, offsets = sr.flatten([cases["noise"], cases["hinge"], cases["invalid"]])
    residue, pair = conditioned("thresholds 0.25, 0.75, 3, 6", ref, mob, offsets, thresholds=limits)
    got = lddt.lddt_arrays(ref, mob, offsets, thresholds=limits, device=gpu)
    assert same_bytes(got.residue, residue) and same_bytes(got.pair, pair)
    default = lddt.lddt_arrays(ref, mob, offsets, device=gpu)
    assert same_bytes(got.residue[:, 0], default.residue[:, 0]) and not same_bytes(got.residue, default.residue)
    unordered = lddt.lddt_arrays(ref, mob, offsets, thresholds=limits[::-1], device=gpu)          # a column belongs to its threshold
    assert same_bytes(unordered.residue[:, 1:], np.ascontiguousarray(got.residue[:, :0:-1]))


def test_non_finite_positions_in_either_list(gpu):
    rng = np.random.default_rng(11)
    ref, mob = sr.synthetic_pair(300, rng)
    ref, mob = ref.copy(), mob.copy()
    bad_ref, bad_mob = rng.choice(300, 12, replace=False), rng.choice(300, 12, replace=False)
    for n, i in enumerate(bad_ref):
        ref[i, n % 3] = (np.nan, np.inf, -np.inf)[n % 3]
    for n, i in enumerate(bad_mob):
        mob[i, (n + 1) % 3] = (np.inf, -np.inf, np.nan)[n % 3]
    mob[0], ref[299] = np.inf, np.nan                                            # whole positions too, first and last
    offsets = np.array([0, 300], np.int64)
    residue, pair = conditioned("NaN and infinities scattered in both lists", ref, mob, offsets)
    got = lddt.lddt_arrays(ref, mob, offsets, device=gpu)
    assert same_bytes(got.residue, residue) and same_bytes(got.pair, pair)
    bad = sorted(set(bad_ref) | set(bad_mob) | {0, 299})
    assert got.pair[0, 0] == 300 - len(bad) and not got.residue[bad].any() and got.pair[0, 1] > 0
    clean = lddt.lddt_arrays(np.delete(ref, bad, axis=0), np.delete(mob, bad, axis=0), [0, 300 - len(bad)], device=gpu)
    assert same_bytes(np.delete(got.residue, bad, axis=0), clean.residue) and same_bytes(got.pair, clean.pair)     # as if they were absent


def test_files_and_cli_end_to_end(gpu, golden, cases, tmp_path, capsys):
    import analyse_models
    names = ("rigid", "noise", "hinge", "mirror")
    (tmp_path / "models" / "deep").mkdir(parents=True)
    (tmp_path / "native.pdb").write_text(sr.pdb_text(cases["hinge"][0]))
    for name in names:
        (tmp_path / "models" / "deep" / f"{name}.pdb").write_text(sr.pdb_text(cases[name][1]))
    ok = np.isfinite(cases["invalid"][0]).all(axis=1) & np.isfinite(cases["invalid"][1]).all(axis=1)
    numbers = np.arange(1, 77)[ok]
    text = sr.pdb_text(cases["invalid"][1][ok]).splitlines()
    (tmp_path / "models" / "invalid.pdb").write_text("\n".join(line[:22] + f"{n:4d}" + line[26:60] + f"{50.0 + n:6.2f}" + line[66:]
                                                               for line, n in zip(text, numbers)) + "\nEND\n")      # numbered as the native, B = 50 + n
    listed = [(tmp_path / "native.pdb", tmp_path / "models" / "deep" / f"{name}.pdb") for name in names] + [(tmp_path / "native.pdb", tmp_path / "models" / "invalid.pdb")]
    stats = {}
    results = lddt.lddt(listed, device=gpu, stats=stats)
    assert stats["submissions"] == 1 and stats["files_parsed"] == 6 and stats["kernel_ms"] > 0
    native = np.round(cases["hinge"][0], 3)
    arrays = [(native, np.round(cases[name][1], 3)) for name in names]
    ref, mob, offsets = sr.flatten(arrays)
    residue, pair = conditioned("1ubq cases at three decimals", ref, mob, offsets)
    for k, res in enumerate(results[:4]):
        rows = residue[76 * k:76 * k + 76].astype(np.int64)
        assert res.error is None and (res.n_valid, res.n_included) == (76, int(pair[k, 1])) and res.n_i.tolist() == rows[:, 0].tolist()
        assert res.lddt == lr.score(pair[k]) and res.preserved == tuple(int(c) / int(pair[k, 1]) for c in pair[k, 2:])
        assert res.lddt_i.tolist() == [int(r[1:].sum()) / (4 * int(r[0])) for r in rows] and (res.model_bfactor == 0.0).all()
    assert results[0].lddt > 0.999 and results[3].lddt > 0.999 and abs(results[2].lddt - lr.score(golden["hinge_pair"])) < 5e-3
    assert "length mismatch" in results[4].error
    (numbered,) = lddt.lddt([listed[4]], pair_by="number", device=gpu)
    want = conditioned("invalid case by number", native[ok], np.round(cases["invalid"][1][ok], 3), np.array([0, 73]))
    assert numbered.error is None and (numbered.unpaired_reference, numbered.unpaired_model) == (3, 0) and numbered.n_valid == 73
    assert numbered.n_i.tolist() == want[0][:, 0].tolist() and numbered.lddt == lr.score(want[1][0])
    assert [r.number for r in numbered.residues] == [str(n) for n in numbers] and numbered.model_bfactor.tolist() == (50.0 + numbers).tolist()
    # the command line: by position, then by number
    out = tmp_path / "out"
    parser = analyse_models.build_parser()
    common = ["--path_to_reference", str(tmp_path / "native.pdb"), "--path_to_models", str(tmp_path / "models"), "--device", str(gpu)]
    analyse_models.main(parser.parse_args(common + ["--path_to_output", str(out), "--lddt"]))
    assert "5 pairs (1 with an error), 304 positions, 6 files parsed in 2 GPU submission(s)" in capsys.readouterr().out

    def read(folder, name):
        with open(folder / name, newline="") as f:
            return list(csv.reader(f))
    scores, per = read(out, "model_lddt.csv"), read(out, "residue_lddt.csv")
    assert scores[0] == analyse_models.LDDT_COLUMNS and per[0] == analyse_models.RESIDUE_LDDT_COLUMNS and len(per) == 1 + 4 * 76
    assert [r[0] for r in scores[1:]] == ["deep/hinge.pdb", "deep/mirror.pdb", "deep/noise.pdb", "deep/rigid.pdb", "invalid.pdb"]
    row = dict(zip(scores[0], scores[1]))
    hinge = results[2]
    assert float(row["lddt"]) == hinge.lddt and int(row["n_included"]) == hinge.n_included and row["mean_model_bfactor"] == "0.0"
    assert [float(row[f"preserved_{t}"]) for t in ("0.5", "1", "2", "4")] == list(hinge.preserved)
    assert [float(r[5]) for r in per[1:77]] == hinge.lddt_i.tolist() and [int(r[4]) for r in per[1:77]] == hinge.n_i.tolist()
    assert {r[3] for r in per[1:]} == {"GLY"} and "length mismatch" in scores[5][-1]
    plain = tmp_path / "plain"
    analyse_models.main(parser.parse_args(common + ["--path_to_output", str(plain)]))
    assert sorted(p.name for p in plain.iterdir()) == ["model_scores.csv", "residue_deviation.csv"]
    for name in ("model_scores.csv", "residue_deviation.csv"):
        assert (out / name).read_bytes() == (plain / name).read_bytes()
    by_number = tmp_path / "by_number"
    analyse_models.main(parser.parse_args(common + ["--path_to_output", str(by_number), "--lddt", "--pair_by", "number"]))
    scores, per = read(by_number, "model_lddt.csv"), read(by_number, "residue_lddt.csv")
    last = dict(zip(scores[0], scores[5]))
    assert last["error"] == "" and float(last["lddt"]) == numbered.lddt and int(last["n_valid"]) == 73 and len(per) == 1 + 4 * 76 + 73
    assert float(last["mean_model_bfactor"]) == float(np.mean(50.0 + numbers)) and [float(r[6]) for r in per[-73:]] == (50.0 + numbers).tolist()
    assert scores[1][3:] == [str(v) for v in row.values()][3:]                  # numbered alike: pairing by number gives the same row
