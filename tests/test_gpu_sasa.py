"""th_sasa on the GPU against the NumPy restatement (tests/sasa_restatement.py) and the committed fixture.  Everything — counts, masks
and totals — is compared AS BYTES.

That is fair only if both sides compute the same doubles.  The decisions are s < t*t and d < R_j*R_j, strict, on float64 sums of
products; every product, sum and difference of the rule is written out with its order and is rounded on its own on both sides (no
fused multiply-add, no roots, no divisions), the points are an input that both sides read, and the result is an AND over neighbours,
which no order of evaluation can change: there is no tolerance to choose.  Areas are host arithmetic on those integers, the same
operations on both sides, and are compared with == as well."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sasa_restatement as sr  # noqa: E402
from test_sasa_host import dimer_model  # noqa: E402
from timed_hip import sasa  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return np.load(sr.GOLDEN)


@pytest.fixture(scope="module")
def inputs(golden):
    return sr.cases(golden["points_96"], golden["points_960"])


@pytest.fixture(scope="module")
def lengths():
    """the length batch flattened and its restatement at every number of points: computed once, shared, never changed"""
    flat = sr.flatten(sr.length_batch())
    points = {n: sasa.sphere_points(n) for n in sr.BATCH_POINTS}
    return flat, points, {n: sr.restate_batch(*flat, sr.PROBE, points[n]) for n in sr.BATCH_POINTS}


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check(got, want, what=""):
    exposed, mask, totals = want
    assert same_bytes(got.exposed, exposed), (what, np.argwhere(got.exposed != exposed)[:8].tolist())
    assert same_bytes(got.structure, totals), (what, got.structure.tolist(), totals.tolist())
    if got.mask is not None:
        assert same_bytes(got.mask, mask), (what, np.argwhere(got.mask != mask)[:8].tolist())


def settings(inputs):
    """the cases grouped by what one call fixes: the probe and the points"""
    groups = {}
    for name in sr.CASES:
        _, _, probe, points = inputs[name]
        groups.setdefault((probe, points.tobytes()), []).append(name)
    return list(groups.values())


def test_golden_cases_in_one_batch_alone_and_in_any_order(gpu, golden, inputs):
    assert golden["cases"].tolist() == list(sr.CASES)
    groups = settings(inputs)
    assert sorted(len(g) for g in groups) == [1, 1, 1, 2, 2, 4]
    for names in groups:
        probe, points = inputs[names[0]][2:]
        parts = [inputs[name] for name in names]
        flat = sr.flatten(parts)
        got = sasa.sasa_arrays(*flat, probe=probe, points=points, device=gpu, mask=True)
        assert got.exposed.dtype == np.int32 and got.mask.dtype == np.uint64 and got.structure.dtype == np.int64
        assert got.mask.shape == (len(flat[0]), sasa.mask_words(len(points)))
        for k, name in enumerate(names):
            a, b = int(flat[2][k]), int(flat[2][k + 1])
            print(name, got.structure[k].tolist())
            assert same_bytes(got.exposed[a:b], golden[f"{name}_exposed"]) and same_bytes(got.mask[a:b], golden[f"{name}_mask"]), name
            assert same_bytes(got.structure[k], golden[f"{name}_totals"]), name
            alone = sasa.sasa_arrays(*sr.flatten([parts[k]]), probe=probe, points=points, device=gpu, mask=True)
            assert same_bytes(alone.exposed, got.exposed[a:b]) and same_bytes(alone.mask, got.mask[a:b]) and same_bytes(alone.structure[0], got.structure[k])
            if name in sr.ANALYTIC:
                assert alone.exposed.tolist() == sr.ANALYTIC[name], name
        order = np.random.default_rng(5).permutation(len(parts))
        shuffled = sasa.sasa_arrays(*sr.flatten([parts[k] for k in order]), probe=probe, points=points, device=gpu, mask=True)
        at = 0
        for k in order:
            n = len(parts[k][0])
            assert same_bytes(shuffled.exposed[at:at + n], golden[f"{names[k]}_exposed"]) and same_bytes(shuffled.mask[at:at + n], golden[f"{names[k]}_mask"])
            at += n
        assert same_bytes(shuffled.structure, got.structure[order])


@pytest.mark.parametrize("n_points", sr.BATCH_POINTS)
def test_every_length_in_one_batch(gpu, lengths, n_points):
    flat, points, restated = lengths
    want = restated[n_points]
    exposed, mask, totals = want
    assert np.diff(flat[2]).tolist() == list(sr.BATCH_LENGTHS) * 2
    assert any(o % 2 for o in flat[2].tolist()) and any(o % 64 for o in flat[2].tolist())            # structures start at odd offsets
    # on the restatement first: buried, partly exposed and fully exposed atoms
    print("length batch at", n_points, "points:", totals.sum(axis=0).tolist())
    assert (exposed == 0).sum() > 100 and (exposed == n_points).sum() >= 2 and (n_points < 3 or ((exposed > 0) & (exposed < n_points)).sum() > 100)
    got = sasa.sasa_arrays(*flat, probe=sr.PROBE, points=points[n_points], device=gpu, mask=True)
    check(got, want, f"length batch at {n_points} points")
    again = sasa.sasa_arrays(*flat, probe=sr.PROBE, points=points[n_points], device=gpu, mask=True)   # a second call: the same bytes
    assert same_bytes(again.exposed, got.exposed) and same_bytes(again.mask, got.mask) and same_bytes(again.structure, got.structure)
    timing = {}
    counts = sasa.sasa_arrays(*flat, probe=sr.PROBE, points=points[n_points], device=gpu, timing=timing)    # mask_out = NULL: the same counts
    assert counts.mask is None
    check(counts, want, "without the mask")
    assert timing["kernel_ms"] > 0 and abs(timing["points_ms"] + timing["totals_ms"] - timing["kernel_ms"]) < 1e-9
    # a structure alone gives the bytes it has in the batch: 257 atoms of 1ubq and 65 of the box
    for k in (8, 15):
        a, b = int(flat[2][k]), int(flat[2][k + 1])
        alone = sasa.sasa_arrays(flat[0][a:b], flat[1][a:b], [0, b - a], probe=sr.PROBE, points=points[n_points], device=gpu, mask=True)
        assert same_bytes(alone.exposed, exposed[a:b]) and same_bytes(alone.mask, mask[a:b]) and same_bytes(alone.structure[0], totals[k])


def test_hostile_inputs(gpu, golden):
    points = golden["points_96"]
    rng = np.random.default_rng(9)
    xyz, radius = sr.ubq_atoms()[:2]
    parts = []
    parts.append((np.array([10.0, 20.0, 30.0]) + rng.uniform(-1e-3, 1e-3, (300, 3)), np.full(300, 1.7)))     # 300 atoms on one spot: no capacity
    parts.append(sr.box_atoms(600, rng, side=10.0))                                                          # 600 atoms in a 10 Angstrom cube
    holed, bad_radius = xyz.copy(), radius.copy()
    for n, i in enumerate(rng.choice(np.arange(1, 601), 12, replace=False)):
        holed[i, n % 3] = (np.nan, np.inf, -np.inf)[n % 3]
    holed[0], holed[601] = np.nan, np.inf                                                                    # the whole first and last atom
    parts.append((holed, radius))
    for n, i in enumerate(rng.choice(602, 12, replace=False)):
        bad_radius[i] = (0.0, -1.0, np.nan, -1.4, np.inf, -np.inf)[n % 6]          # 0 and -1 leave R = 1.4 and 0.4: valid; -1.4: R = 0 exactly
    parts.append((xyz, bad_radius))
    far = xyz.copy()
    far[::7] *= 1e200                                                                                        # differences overflow: not near
    parts.append((far, radius))
    parts.append((np.zeros((2, 3)), np.array([1.7, 1.7])))                                                   # coincident atoms of equal radius
    flat = sr.flatten(parts)
    want = sr.restate_batch(*flat, sr.PROBE, points)
    print("hostile totals", want[2].tolist())
    assert want[2][0].tolist()[0] == 300 and want[2][1][1] > 300 and want[2][2][0] == 602 - 14 and want[2][3][0] == 602 - 8
    assert (want[0][flat[2][4]:flat[2][5]][::7] == 96).all() and 0 < want[0][-1] == want[0][-2] < 96
    got = sasa.sasa_arrays(*flat, probe=sr.PROBE, points=points, device=gpu, mask=True)
    check(got, want, "hostile inputs")
    invalid = want[0] < 0
    assert invalid.sum() == 22 and not got.mask[invalid].any() and (got.exposed[invalid] == -1).all()
    # R_i <= 0 through a negative probe: every atom invalid, nothing exposed, nothing occluded
    negative = sasa.sasa_arrays(xyz, radius, [0, 602], probe=-1.9, points=points, device=gpu, mask=True)
    check(negative, sr.restate_batch(xyz, radius, np.array([0, 602]), -1.9, points), "probe -1.9")
    assert (negative.exposed == -1).all() and not negative.mask.any() and negative.structure.tolist() == [[0, 0, 0]]
    partly = sasa.sasa_arrays(xyz, radius, [0, 602], probe=-1.6, points=points, device=gpu)                  # only C, S survive: R = 0.1, 0.2
    check(partly, sr.restate_batch(xyz, radius, np.array([0, 602]), -1.6, points), "probe -1.6")
    assert 0 < partly.structure[0, 0] < 602
    nan_probe = sasa.sasa_arrays(xyz, radius, [0, 602], probe=float("nan"), points=points, device=gpu)
    assert (nan_probe.exposed == -1).all()


def test_files_end_to_end(gpu, golden):
    stats = {}
    (one, two) = sasa.sasa([sr.UBQ, sr.UBQ], device=gpu, stats=stats)
    assert stats["submissions"] == 1 and stats["files_parsed"] == 2 and stats["kernel_ms"] > 0
    assert one.error is None and same_bytes(one.exposed, golden["ubq_exposed"]) and same_bytes(two.exposed, golden["ubq_exposed"])
    assert same_bytes(one.residue_area, golden["ubq_residue_area"][0]) and same_bytes(one.polar_area, golden["ubq_residue_area"][1])
    assert same_bytes(one.apolar_area, golden["ubq_residue_area"][2]) and same_bytes(one.backbone_area, golden["ubq_residue_area"][3])
    assert [one.total_area, one.total_polar_area, one.total_apolar_area] == golden["ubq_area"].tolist()
    assert (one.n_atoms, one.n_buried_atoms, one.counts) == (602, 271, (24, 35, 17)) and [r.number for r in one.residues] == [str(k) for k in range(1, 77)]
    stats = {}
    dimer = sasa.sasa([dimer_model()], device=gpu, interface=True, mask=True, stats=stats)[0]
    assert stats["submissions"] == 1 and same_bytes(dimer.exposed, golden["ubq_dimer_exposed"]) and same_bytes(dimer.mask, golden["ubq_dimer_mask"])
    assert dimer.interface_area == float(golden["ubq_dimer_interface"]) > 0 and same_bytes(dimer.area_lost, golden["ubq_dimer_area_lost"])
    from design_utils.analyse_utils import extract_sasa_from_ampal
    assert extract_sasa_from_ampal(sr.UBQ, device=gpu) == [golden["ubq_residue_area"][0].tolist()]


def test_both_command_lines_end_to_end(gpu, tmp_path, capsys, golden):
    import csv
    import gzip

    import analyse_models
    import analyse_properties
    with gzip.open(sr.UBQ, "rt") as f:
        text = f.read()
    (tmp_path / "models").mkdir()
    (tmp_path / "native.pdb").write_text(text)
    (tmp_path / "models" / "same.pdb").write_text(text)
    plain, out = tmp_path / "plain", tmp_path / "properties"
    common = ["--path_to_pdb", str(tmp_path / "native.pdb"), "--device", str(gpu)]
    analyse_properties.main(analyse_properties.build_parser().parse_args(common + ["--path_to_output", str(plain)]))
    analyse_properties.main(analyse_properties.build_parser().parse_args(common + ["--path_to_output", str(out), "--sasa"]))
    assert sorted(p.name for p in plain.iterdir()) == ["residue_properties.csv", "structure_properties.csv"]
    assert sorted(p.name for p in out.iterdir()) == ["residue_properties.csv", "residue_sasa.csv", "structure_properties.csv", "structure_sasa.csv"]
    assert all((out / p.name).read_bytes() == p.read_bytes() for p in plain.iterdir())
    with open(out / "residue_sasa.csv", newline="") as f:
        rows = list(csv.reader(f))
    with open(out / "structure_sasa.csv", newline="") as f:
        header, whole = list(csv.reader(f))
    row = dict(zip(header, whole))
    assert [float(r[4]) for r in rows[1:]] == golden["ubq_residue_area"][0].tolist() and "".join(r[9] for r in rows[1:]).count("C") == 24
    assert [float(row[k]) for k in ("total_area", "polar_area", "apolar_area")] == golden["ubq_area"].tolist()
    assert [int(row[k]) for k in ("atoms", "residues", "n_core", "n_boundary", "n_surface", "buried_atoms")] == [602, 76, 24, 35, 17, 271]
    capsys.readouterr()
    common = ["--path_to_reference", str(tmp_path / "native.pdb"), "--path_to_models", str(tmp_path / "models"), "--device", str(gpu)]
    bare, scores = tmp_path / "bare", tmp_path / "scores"
    analyse_models.main(analyse_models.build_parser().parse_args(common + ["--path_to_output", str(bare)]))
    capsys.readouterr()
    analyse_models.main(analyse_models.build_parser().parse_args(common + ["--path_to_output", str(scores), "--sasa"]))
    assert "2 files parsed in 2 GPU submission(s)" in capsys.readouterr().out
    assert sorted(p.name for p in bare.iterdir()) == ["model_scores.csv", "residue_deviation.csv"]
    assert sorted(p.name for p in scores.iterdir()) == ["model_sasa.csv", "model_scores.csv", "residue_deviation.csv", "residue_sasa.csv"]
    assert all((scores / p.name).read_bytes() == p.read_bytes() for p in bare.iterdir())
    with open(scores / "model_sasa.csv", newline="") as f:
        header, row = list(csv.reader(f))
    got = dict(zip(header, row))
    assert (got["n_paired"], got["burial_agreement"], got["mean_abs_rsa_difference"], got["error"]) == ("76", "1.0", "0.0", "")
    assert float(got["reference_total_area"]) == float(got["model_total_area"]) == float(golden["ubq_area"][0])
    assert float(got["model_apolar_area"]) == float(golden["ubq_area"][2])
