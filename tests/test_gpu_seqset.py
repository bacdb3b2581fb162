"""th_seqset on the GPU against the committed fixture (tests/golden/seqset_golden.npz, made by the NumPy restatement
tests/seqset_restatement.py from the rule, not by the kernel).  Every table — per sequence, per position, per set and the matrix — is
compared AS BYTES: everything the kernel computes is an integer count, a maximum or a minimum of integers, so there is no tolerance to
choose and no order of evaluation that could change a bit."""
import csv
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seqset_restatement as qr  # noqa: E402
from timed_hip import seqset  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return np.load(qr.GOLDEN)


@pytest.fixture(scope="module")
def inputs(golden):
    """name -> (codes, native or None, min_matches), from the fixture's own arrays"""
    out = {}
    for name in qr.CASES:
        native = golden[f"{name}_native"]
        out[name] = (golden[f"{name}_codes"], native if native.size else None, int(golden[f"{name}_min_matches"]))
    return out


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def run(parts, gpu, matrix=True, timing=None):
    codes, offsets, lengths, native, thresholds = qr.flatten(parts)
    return seqset.seqset_arrays(codes, offsets, lengths, native, thresholds, matrix=matrix, device=gpu, timing=timing), offsets, lengths


def check(got, offsets, lengths, names, golden, matrix=True):
    at_pos = at_matrix = 0
    for k, name in enumerate(names):
        a, b, length = int(offsets[k]), int(offsets[k + 1]), int(lengths[k])
        n = b - a
        want = golden[f"{name}_seq"]
        assert same_bytes(got.seq[a:b], want), (name, np.argwhere(got.seq[a:b] != want)[:8].tolist())
        assert same_bytes(got.profile[at_pos:at_pos + length], golden[f"{name}_profile"]), name
        assert same_bytes(got.sets[k], golden[f"{name}_set"]), (name, got.sets[k].tolist(), golden[f"{name}_set"].tolist())
        if matrix:
            assert same_bytes(got.matrix[at_matrix:at_matrix + n * n].reshape(n, n), golden[f"{name}_matrix"]), name
        at_pos += length
        at_matrix += n * n


def test_the_fixture_crosses_the_tiles_of_this_build(lib, inputs):
    rows, cols, chunk = seqset.tiles()
    shapes = [codes.shape for codes, _, _ in inputs.values()]
    assert any(n > 2 * rows and n % rows and n > 2 * cols and n % cols for n, _ in shapes), (rows, cols, shapes)      # more than two tiles, not a multiple
    assert any(rows < n < 2 * rows and cols < n < 2 * cols for n, _ in shapes)                                         # a partial second tile
    assert any(length > chunk and length % chunk and length % 4 for _, length in shapes), (chunk, shapes)             # more than one chunk, and the pad
    assert any(length % 4 and length < chunk for _, length in shapes) and any(n == 0 for n, _ in shapes) and any(n == 1 for n, _ in shapes)


def test_all_cases_in_one_call_equal_the_fixture_as_bytes(gpu, golden, inputs):
    assert golden["cases"].tolist() == list(qr.CASES)
    timing = {}
    got, offsets, lengths = run([inputs[name] for name in qr.CASES], gpu, timing=timing)
    assert got.seq.dtype == np.int32 and got.profile.dtype == np.int32 and got.sets.dtype == np.int64 and got.matrix.dtype == np.int32
    for k, name in enumerate(qr.CASES):
        print(name, got.sets[k].tolist())
    check(got, offsets, lengths, qr.CASES, golden)
    assert math.isfinite(timing["kernel_ms"]) and timing["kernel_ms"] > 0 and 0 < timing["cluster_ms"] < timing["kernel_ms"]
    # without the matrix every other table keeps its bytes; without clustering and without a native only their columns change
    plain, _, _ = run([inputs[name] for name in qr.CASES], gpu, matrix=False)
    assert plain.matrix is None and same_bytes(plain.seq, got.seq) and same_bytes(plain.profile, got.profile) and same_bytes(plain.sets, got.sets)
    codes, offsets, lengths, native, thresholds = qr.flatten([inputs[name] for name in qr.CASES])
    bare = seqset.seqset_arrays(codes, offsets, lengths, None, None, device=gpu)
    assert same_bytes(bare.seq[:, 3:7], got.seq[:, 3:7]) and not bare.seq[:, :3].any() and (bare.seq[:, 7] == -1).all()
    assert same_bytes(bare.profile, got.profile) and same_bytes(bare.sets[:, :2], got.sets[:, :2]) and (bare.sets[:, 2] == -1).all() and not bare.sets[:, 3].any()
    # the matrix: symmetric, L on the diagonal
    at = 0
    for k, name in enumerate(qr.CASES):
        n = int(offsets[k + 1] - offsets[k])
        square = got.matrix[at:at + n * n].reshape(n, n)
        assert np.array_equal(square, square.T) and (np.diag(square) == lengths[k]).all(), name
        at += n * n


@pytest.mark.parametrize("name", qr.CASES)
def test_each_case_alone(gpu, golden, inputs, name):
    got, offsets, lengths = run([inputs[name]], gpu)
    check(got, offsets, lengths, [name], golden)


def test_a_set_keeps_its_bytes_wherever_it_sits(gpu, golden, inputs):
    for names in (("ubq_drift", "two_tiles", "long"), ("single", "ubq_drift", "all_same"), ("empty", "long", "two_tiles", "ubq_drift")):
        got, offsets, lengths = run([inputs[name] for name in names], gpu)
        check(got, offsets, lengths, names, golden)


def test_analyse_over_three_submissions_equals_one(gpu, golden, inputs):
    names = ("ubq_drift", "two_tiles", "all_same", "single", "long")
    sets = [inputs[name][0] for name in names]
    natives = [inputs[name][1] for name in names]
    one, three = {}, {}
    whole = seqset.analyse(sets, natives, cluster_identity=0.8, matrix=True, device=gpu, stats=one)
    budget = seqset.set_bytes(130, 9, True) + seqset.set_bytes(66, 4, True) + seqset.set_bytes(1, 5, True)
    assert seqset.set_bytes(70, 76, True) <= budget < seqset.set_bytes(70, 76, True) + seqset.set_bytes(130, 9, True)
    split = seqset.analyse(sets, natives, cluster_identity=0.8, matrix=True, device=gpu, budget_bytes=budget, stats=three)
    assert one["submissions"] == 1 and three["submissions"] == 3 and one["kernel_ms"] > 0
    for a, b in zip(whole, split):
        assert a.error is None and same_bytes(a.seq, b.seq) and same_bytes(a.profile, b.profile) and same_bytes(a.totals, b.totals) and same_bytes(a.matrix, b.matrix)
    drift, two = whole[0], whole[1]
    assert same_bytes(drift.seq, golden["ubq_drift_seq"]) and drift.min_matches == 61 and drift.n_clusters == int(golden["ubq_drift_set"][2])
    assert drift.representatives.tolist() == np.flatnonzero(golden["ubq_drift_seq"][:, 7] == np.arange(70)).tolist()
    assert np.isnan(two.identity_to_native).all() and not two.seq[:, :3].any() and two.n_distinct == int(golden["two_tiles_set"][1])
    assert drift.identity_to_native.tolist() == (golden["ubq_drift_seq"][:, 0] / 76.0).tolist()
    from design_utils.analyse_utils import calculate_sequence_identity, calculate_sequence_similarity
    native, draw = seqset.decode(inputs["ubq_drift"][1]), seqset.decode(inputs["ubq_drift"][0][0])
    assert calculate_sequence_identity(native, draw, device=gpu) == drift.identity_to_native[0]
    assert calculate_sequence_similarity(native, draw, device=gpu) == drift.similarity_to_native[0]


def test_analyse_samples_end_to_end(gpu, tmp_path, inputs, golden):
    import analyse_samples
    drift, native, _ = inputs["ubq_drift"]
    two = inputs["two_tiles"][0]
    with open(tmp_path / "draws.fasta", "w") as f:
        f.writelines(f">1ubq_A_{n}\n{seqset.decode(row)}\n" for n, row in enumerate(drift))
        f.writelines(f">toy_{n}\n{seqset.decode(row)}\n" for n, row in enumerate(two))
        f.write(">ragged_0\nACD\n>ragged_1\nACDE\n")
    with open(tmp_path / "native.fasta", "w") as f:
        f.write(f">1ubq_A\n{seqset.decode(native)}\n")
    common = ["--path_to_samples", str(tmp_path / "draws.fasta"), "--path_to_native_fasta", str(tmp_path / "native.fasta"), "--cluster_identity", "0.8",
              "--device", str(gpu)]
    first = analyse_samples.main(analyse_samples.build_parser().parse_args(common + ["--path_to_output", str(tmp_path / "a")]))
    second = analyse_samples.main(analyse_samples.build_parser().parse_args(common + ["--path_to_output", str(tmp_path / "b")]))
    names = ["sample_scores.csv", "set_scores.csv", "position_profile.csv", "representatives.fasta"]
    assert [os.path.basename(p) for p in first] == names and sorted(p.name for p in (tmp_path / "a").iterdir()) == sorted(names)
    for a, b in zip(first, second):
        assert open(a, "rb").read() == open(b, "rb").read(), a
    with open(first[1], newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == analyse_samples.SET_COLUMNS and [r[0] for r in rows[1:]] == ["1ubq_A", "toy", "ragged"]
    ubq, toy, ragged = (dict(zip(rows[0], r)) for r in rows[1:])
    want = golden["ubq_drift_set"]
    assert (ubq["n"], ubq["length"], ubq["n_distinct"], ubq["n_clusters"], ubq["min_matches"], ubq["error"]) == ("70", "76", "68", str(int(want[2])), "61", "")
    assert float(ubq["mean_identity_to_native"]) == float(want[3]) / (70 * 76) and float(ubq["mean_pairwise_identity"]) == float(want[0]) / (70 * 69 // 2 * 76)
    assert toy["mean_identity_to_native"] == "" and toy["error"] == "" and "unequal lengths" in ragged["error"] and ragged["n"] == "2"
    with open(first[0], newline="") as f:
        draws = list(csv.reader(f))
    assert draws[0] == analyse_samples.SAMPLE_COLUMNS and len(draws) == 1 + 70 + 130
    assert [int(r[11]) for r in draws[1:71]] == golden["ubq_drift_seq"][:, 7].tolist() and draws[6][2] == "1ubq_A_5" and draws[6][9:11] == ["2", "0"]
    with open(first[2], newline="") as f:
        profile = list(csv.reader(f))
    assert len(profile) == 1 + 76 + 9 and [[int(v) for v in r[6:]] for r in profile[1:77]] == golden["ubq_drift_profile"].tolist()
    fasta = open(first[3]).read().splitlines()
    reps = np.flatnonzero(golden["ubq_drift_seq"][:, 7] == np.arange(70))
    assert fasta[0] == ">1ubq_A_0" and fasta[1] == seqset.decode(drift[0]) and [l for l in fasta if l.startswith(">1ubq_A_")] == [f">1ubq_A_{i}" for i in reps]
    with_matrix = analyse_samples.main(analyse_samples.build_parser().parse_args(common + ["--path_to_output", str(tmp_path / "c"), "--matrix"]))
    assert [os.path.basename(p) for p in with_matrix[4:]] == ["1ubq_A_identity.csv", "toy_identity.csv"]
    assert np.array_equal(np.loadtxt(with_matrix[4], delimiter=",", dtype=np.int32), golden["ubq_drift_matrix"])
    for a, b in zip(first, with_matrix[:4]):
        assert open(a, "rb").read() == open(b, "rb").read(), a


def test_more_representatives_than_one_round_of_the_cluster_kernel(gpu):
    """k_seqset_cluster shares the representatives out 1 024 at a time: 1 100 draws far from one another, so that nearly all become
    representatives, with copies that must join a representative of the second round, and one that matches a representative of
    either round and must take the lower"""
    rng = np.random.default_rng(3)
    codes = rng.integers(0, 20, (1100, 70)).astype(np.uint8)           # 70 residues: one whole block of 16 dwords and a tail
    codes[1090] = codes[1060]                                          # equal to a representative of the second round
    codes[1095] = codes[1070]
    codes[1095, :5] = (codes[1070, :5] + 1) % 20                       # 65 of 70 with it: joins at 63
    codes[1050] = codes[10]                                            # the first round again, far down the list
    codes[1099, :35] = codes[7, :35]                                   # half of a first-round and half of a second-round representative:
    codes[1099, 35:] = codes[1080, 35:]                                # below the threshold for both
    threshold = 63
    want = qr.restate(codes, None, threshold)
    reps = np.flatnonzero(want["seq"][:, 7] == np.arange(1100))
    assert len(reps) == 1097 and want["seq"][[1050, 1090, 1095, 1099], 7].tolist() == [10, 1060, 1070, 1099]
    got = seqset.seqset_arrays(codes.reshape(-1), [0, 1100], [70], None, [threshold], device=gpu)
    assert same_bytes(got.seq, want["seq"]) and same_bytes(got.sets[0], want["set"]) and same_bytes(got.profile, want["profile"])
    loose = qr.restate(codes[-160:], None, 10)                         # a threshold most pairs miss and some meet
    assert 100 < loose["set"][2] < 150
    again = seqset.seqset_arrays(codes[-160:].reshape(-1), [0, 160], [70], None, [10], device=gpu)
    assert same_bytes(again.seq, loose["seq"]) and same_bytes(again.sets[0], loose["set"])
