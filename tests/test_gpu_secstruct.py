"""th_secondary_structure on the GPU against the NumPy restatement (tests/secstruct_restatement.py) and the committed fixture.
Everything — classes, residue tables, totals and the hydrogen-bond bitmaps — is compared AS BYTES.

That is fair only if no decision sits on an edge.  The decisions are e < -500 on an integer energy, the CA test s < 81, the link test
s <= 6.25 and the bend's cosine against cos 70; every float64 operation of the rule is written out with its order and is rounded on
its own on both sides (correctly rounded square roots and divisions, no fused multiply-add), so the two sides compute the same
doubles and not merely close ones: there is no tolerance to choose."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import secstruct_restatement as ss  # noqa: E402
from timed_hip import secstruct  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return np.load(ss.GOLDEN)


@pytest.fixture(scope="module")
def inputs():
    return ss.cases()


@pytest.fixture(scope="module")
def lengths():
    """the length batch flattened and its restatement: computed once, shared, never changed"""
    parts = ss.length_batch()
    flat = ss.flatten(parts)
    return parts, flat, ss.restate_batch(*flat)


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check(got, want, what=""):
    cls, residue, totals, bits = want
    assert same_bytes(got.cls, cls), (what, ss.as_string(got.cls), ss.as_string(cls))
    assert same_bytes(got.residue, residue), (what, np.argwhere(got.residue != residue)[:8].tolist())
    assert same_bytes(got.structure, totals), (what, got.structure.tolist(), totals.tolist())
    if got.bits is not None:
        assert same_bytes(got.bits, bits), what


def test_golden_cases_in_one_batch_alone_and_in_any_order(gpu, golden, inputs):
    assert golden["cases"].tolist() == list(ss.CASES)
    parts = [inputs[name] for name in ss.CASES]
    flat = ss.flatten(parts)
    got = secstruct.secondary_structure_arrays(*flat, device=gpu, bits=True)
    assert got.cls.dtype == np.uint8 and got.residue.dtype == np.int32 and got.structure.dtype == np.int64 and got.bits.dtype == np.uint64
    words = np.concatenate([[0], np.cumsum(secstruct.bitmap_words(np.diff(flat[3])))])
    for k, name in enumerate(ss.CASES):
        a, b = int(flat[3][k]), int(flat[3][k + 1])
        print(name, got.structure[k].tolist(), ss.as_string(got.cls[a:b]))
        assert ss.as_string(got.cls[a:b]) == ss.STRINGS[name], name
        assert same_bytes(got.cls[a:b], golden[f"{name}_cls"]) and same_bytes(got.residue[a:b], golden[f"{name}_residue"]), name
        assert same_bytes(got.structure[k], golden[f"{name}_totals"]) and same_bytes(got.bits[words[k]:words[k + 1]], golden[f"{name}_bits"]), name
        alone = secstruct.secondary_structure_arrays(*ss.flatten([parts[k]]), device=gpu, bits=True)
        assert same_bytes(alone.cls, got.cls[a:b]) and same_bytes(alone.residue, got.residue[a:b]) and same_bytes(alone.structure[0], got.structure[k])
        assert same_bytes(alone.bits, got.bits[words[k]:words[k + 1]]), name
    assert got.structure[0].tolist()[:2] == [76, 54]
    order = np.random.default_rng(5).permutation(len(parts))
    shuffled = secstruct.secondary_structure_arrays(*ss.flatten([parts[k] for k in order]), device=gpu, bits=True)
    at = 0
    for k in order:
        n = len(parts[k][0])
        assert same_bytes(shuffled.cls[at:at + n], golden[f"{ss.CASES[k]}_cls"]) and same_bytes(shuffled.residue[at:at + n], golden[f"{ss.CASES[k]}_residue"])
        at += n
    assert same_bytes(shuffled.structure, got.structure[order])


def test_every_length_in_one_batch(gpu, lengths):
    parts, flat, want = lengths
    cls, residue, totals, bits = want
    assert [len(p[0]) for p in parts] == [0, 1, 2, 4, 5, 6, 63, 64, 65, 128, 129, 256, 257, 300]
    assert any(o % 2 for o in flat[3].tolist()) and any(o % 64 for o in flat[3].tolist())            # structures start at odd offsets
    # on the restatement first: the batch has bonds and at least one each of H, E, G, T and S
    print("length batch totals", totals.sum(axis=0).tolist())
    assert totals[:, 1].sum() > 500 and all(totals[:, 2 + code].sum() > 0 for code in (1, 3, 4, 6, 7))
    assert any(len(set(p[1].tolist())) > 1 for p in parts)                                            # more than one chain id
    got = secstruct.secondary_structure_arrays(*flat, device=gpu, bits=True)
    check(got, want, "length batch")
    again = secstruct.secondary_structure_arrays(*flat, device=gpu, bits=True)                        # a second call: the same bytes
    assert same_bytes(again.cls, got.cls) and same_bytes(again.residue, got.residue) and same_bytes(again.structure, got.structure) and same_bytes(again.bits, got.bits)
    tables = secstruct.secondary_structure_arrays(*flat, device=gpu)                                  # hbond_bits_out = NULL: the same tables
    assert tables.bits is None
    check(tables, want, "without the bitmap")
    timing = {}
    secstruct.secondary_structure_arrays(*flat, device=gpu, timing=timing)
    assert timing["kernel_ms"] > 0 and abs(timing["hbonds_ms"] + timing["assign_ms"] + timing["totals_ms"] - timing["kernel_ms"]) < 1e-9
    # a structure alone gives the bytes it has in the batch: 257 (two tiles, five words) and 65
    for k in (8, 12):
        a, b = int(flat[3][k]), int(flat[3][k + 1])
        alone = secstruct.secondary_structure_arrays(*ss.flatten([parts[k]]), device=gpu)
        assert same_bytes(alone.cls, cls[a:b]) and same_bytes(alone.residue, residue[a:b]) and same_bytes(alone.structure[0], totals[k])


def test_a_donor_nitrogen_exactly_on_an_acceptor_oxygen(gpu, inputs):
    backbone, chain, no_h = (a.copy() for a in inputs["alpha"])
    two = np.concatenate([backbone, backbone + np.array([30.0, 0.0, 0.0])])
    shift = two[5, 3] - two[20 + 12, 0]                                          # move the second helix so that N(32) sits on O(5)
    two[20:] += shift
    two[32, 0] = two[5, 3]                                                       # exactly: the sum above rounds
    assert (two[32, 0] == two[5, 3]).all()
    flat = ss.flatten([(two, np.array([0] * 20 + [1] * 20, np.int32), np.zeros(40, np.uint8))])
    one = ss.restate(two, flat[1], flat[2])
    assert one["taken"][5, 32] and one["energy"][5, 32] == -9900 and one["hb"][5, 32] and one["energy"].min() == -9900
    got = secstruct.secondary_structure_arrays(*flat, device=gpu, bits=True)
    check(got, ss.restate_batch(*flat), "distance 0")
    assert (got.bits[5] >> np.uint64(32)) & np.uint64(1) == 1                    # one word per row: row 5, bit 32


def test_nan_atoms_a_proline_and_a_chain_change(gpu, inputs, lengths):
    parts = []
    rng = np.random.default_rng(9)
    backbone, chain, no_h = lengths[0][-1]                                       # 300 residues of tiled 1ubq
    holed = backbone.copy()
    for n, i in enumerate(rng.choice(300, 12, replace=False)):
        holed[i, n % 4, n % 3] = (np.nan, np.inf, -np.inf)[n % 3]
    holed[0], holed[299] = np.nan, np.inf                                        # whole residues too, first and last
    parts.append((holed, chain, no_h))
    alpha = inputs["alpha"][0]
    proline = np.zeros(20, np.uint8)
    proline[10] = 1
    parts.append((alpha, np.zeros(20, np.int32), proline))
    parts.append((alpha, np.array([3] * 7 + [1] * 13, np.int32), np.zeros(20, np.uint8)))
    parts.append((backbone, np.zeros(300, np.int32), np.ones(300, np.uint8)))    # nobody donates: no bond at all
    flat = ss.flatten(parts)
    want = ss.restate_batch(*flat)
    print("NaN / PRO / chains:", [ss.as_string(want[0][a:b]) for a, b in zip(flat[3][1:3], flat[3][2:4])], want[2].tolist())
    assert want[2][0, 0] < 290 and want[2][0, 1] > 100 and want[2][3, 1] == 0
    assert ss.as_string(want[0][300:320]) == ss.STRINGS["alpha"] and ss.as_string(want[0][320:340]) == "-HHHHH--HHHHHHHHHHH-"
    assert want[1][300 + 10, 4] == 0 and want[2][1, 1] == 15                     # the proline donates nothing: one bond fewer
    got = secstruct.secondary_structure_arrays(*flat, device=gpu, bits=True)
    check(got, want, "NaN atoms, proline, chain change")
    assert got.structure[3, 1] == 0 and not got.bits[-secstruct.bitmap_words(300):].any()
    bad = ~np.isfinite(holed.reshape(300, 12)).all(axis=1)
    assert not got.cls[:300][bad].any() and not (got.residue[:300, 2][bad] & (secstruct.FLAG_VALID | secstruct.FLAG_CONN)).any()
    assert not got.residue[:300, 3:5][bad].any()


def test_files_end_to_end(gpu, golden):
    stats = {}
    (one, two) = secstruct.secondary_structure([ss.UBQ, ss.UBQ], device=gpu, stats=stats)
    assert stats["submissions"] == 1 and stats["files_parsed"] == 2 and stats["kernel_ms"] > 0
    assert one.error is None and one.string == ss.UBQ_STRING and two.string == ss.UBQ_STRING and (one.n_valid, one.n_hbonds) == (76, 54)
    assert same_bytes(one.cls, golden["ubq_cls"]) and same_bytes(one.partners, golden["ubq_residue"][:, :2].copy())
    assert one.counts.tolist() == golden["ubq_totals"][2:].tolist() and [r.number for r in one.residues] == [str(k) for k in range(1, 77)]
    assert secstruct.as_string(one.cls, three=True).count("H") == 18 and abs(sum(one.fractions) - 1.0) < 1e-12


def test_both_command_lines_end_to_end(gpu, tmp_path, capsys):
    import csv
    import gzip

    import analyse_models
    import analyse_properties
    with gzip.open(ss.UBQ, "rt") as f:
        text = f.read()
    (tmp_path / "models").mkdir()
    (tmp_path / "native.pdb").write_text(text)
    (tmp_path / "models" / "same.pdb").write_text(text)
    out = tmp_path / "properties"
    analyse_properties.main(analyse_properties.build_parser().parse_args(["--path_to_pdb", str(tmp_path / "native.pdb"), "--path_to_output", str(out),
                                                                          "--device", str(gpu), "--secondary_structure"]))
    with open(out / "residue_secondary_structure.csv", newline="") as f:
        rows = list(csv.reader(f))
    with open(out / "structure_secondary_structure.csv", newline="") as f:
        whole = list(csv.reader(f))
    assert "".join(r[4] for r in rows[1:]) == ss.UBQ_STRING and [int(v) for v in whole[1][1:11]] == [76, 54, 16, 12, 2, 24, 6, 0, 12, 4]
    scores = tmp_path / "scores"
    analyse_models.main(analyse_models.build_parser().parse_args(["--path_to_reference", str(tmp_path / "native.pdb"), "--path_to_models",
                                                                  str(tmp_path / "models"), "--path_to_output", str(scores), "--device", str(gpu),
                                                                  "--secondary_structure"]))
    assert "2 files parsed in 2 GPU submission(s)" in capsys.readouterr().out
    with open(scores / "model_secstruct.csv", newline="") as f:
        header, row = list(csv.reader(f))
    got = dict(zip(header, row))
    assert (got["n_paired"], got["q8"], got["q3"], got["reference_n_hbonds"], got["model_n_hbonds"], got["error"]) == ("76", "1.0", "1.0", "54", "54", "")
