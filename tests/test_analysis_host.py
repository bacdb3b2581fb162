"""predict.py --output_analysis without a GPU: the NumPy restatement of th_analyse_probs (tests/analysis_restatement.py) against
scipy.stats.entropy and hand-built cases (the rank tie rule, interleaved rotamer columns), the metrics timed_hip.analysis derives
from the integer totals (macro precision / recall, normalize="all", bias) and the BLOSUM62 table."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import analysis_restatement as ar  # noqa: E402
from timed_hip import analysis  # noqa: E402


def test_restated_entropy_equals_scipy():
    from scipy.stats import entropy
    rng = np.random.default_rng(5)
    for k, dtype in ((20, np.float16), (338, np.float16), (1024, np.float32), (7, np.float32)):
        z = rng.standard_normal((300, k)) * 3
        p = np.exp(z - z.max(1, keepdims=True))
        p = (p / p.sum(1, keepdims=True)).astype(dtype)
        p[5, :] = 0
        p[6, : k // 2] = 0
        p[7, :] = p[7, :] * 40                                  # unnormalised rows are normalised by their sum
        _, _, got, _ = ar.restate(p, np.zeros(300, int), np.arange(k) % 20)
        with np.errstate(all="ignore"):
            want = entropy(p.astype(np.float64), base=2, axis=1)
        assert np.isnan(got[5]) and np.isnan(want[5])          # 0 / 0
        ok = ~np.isnan(want)
        assert np.array_equal(ok, ~np.isnan(got))
        np.testing.assert_allclose(got[ok], want[ok], rtol=0, atol=1e-12)


def test_restated_entropy_nan_rows_diverge_from_scipy_only_for_negative_entries():
    from scipy.stats import entropy
    x = np.full((4, 20), 0.05)
    x[0, 3] = np.nan
    x[1, 4] = np.inf
    x[2, 5] = -0.01
    _, _, got, tot = ar.restate(x, [-1] * 4, np.arange(20))
    assert np.isnan(got[:3]).all() and not np.isnan(got[3])
    with np.errstate(all="ignore"):
        want = entropy(x, base=2, axis=1)
    assert np.isnan(want[0]) and np.isnan(want[1]) and want[2] == -np.inf      # the documented divergence: NaN here
    assert tot["n_nonfinite"] == 2 and tot["n_labelled"] == 0


def _row(values, k=20):
    r = np.zeros(k)
    for c, v in values.items():
        r[c] = v
    return r


def test_tie_rule_first_column_wins_at_ranks_0_1_and_2_3():
    # columns = residues (k = 20): equal scores rank by the lower residue index
    x = np.stack([_row({3: 0.3, 7: 0.3, 9: 0.2}),               # 3 and 7 tie at the top: 3 is rank 0, 7 rank 1
                  _row({3: 0.3, 7: 0.3, 9: 0.2}),
                  _row({1: 0.4, 2: 0.2, 11: 0.1, 12: 0.1, 4: 0.1}),   # 4, 11, 12 tie behind ranks 0 and 1: ranks 2, 3, 4
                  _row({1: 0.4, 2: 0.2, 11: 0.1, 12: 0.1, 4: 0.1}),
                  _row({1: 0.4, 2: 0.2, 11: 0.1, 12: 0.1, 4: 0.1}),
                  _row({1: 0.4, 2: 0.2, 11: 0.1, 12: 0.1, 4: 0.1})])
    truth = [3, 7, 4, 11, 12, 0]
    pred, rank, _, tot = ar.restate(x, truth, np.arange(20))
    assert pred.tolist() == [3, 3, 1, 1, 1, 1]
    # residue 0 scores 0 with 14 other zero-scored residues: 2..4 ahead of it by score, the zeros at 5, 6, ... behind it by index
    assert rank.tolist() == [0, 1, 2, 3, 4, 5]
    assert tot["rank_hist"][:6].tolist() == [1, 1, 1, 1, 1, 1]
    m = analysis.metrics_from_totals(tot["confusion"], tot["rank_hist"], tot["n_labelled"], tot["n_nonfinite"], tot["n_similar"], 6)
    assert m["accuracy_1"] == 1 / 6 and m["accuracy_2"] == 2 / 6 and m["accuracy_3"] == 3 / 6 and m["accuracy_5"] == 5 / 6


def test_rotamer_scoring_with_interleaved_columns():
    # 7 columns owned by residues 2, 0, 2, 1, 0, 1, 4 (not contiguous, not ordered); residues 3 and 5..19 own no column
    col = np.array([2, 0, 2, 1, 0, 1, 4])
    x = np.array([[0.1, 0.2, 0.3, 0.1, 0.2, 0.05, 0.05],     # s = {2: .3 (col 2), 0: .2 (col 1), 1: .1 (col 3), 4: .05 (col 6)}
                  [0.3, 0.2, 0.1, 0.1, 0.3, 0.0, 0.0],       # s = {2: .3 (col 0), 0: .3 (col 4 ... first at col 4)}: 2 first
                  [0.2, 0.1, 0.1, 0.3, 0.1, 0.3, 0.0],       # residue 1 scores .3 at col 3; residue 4 scores 0
                  [0.2, 0.1, 0.1, 0.3, 0.1, 0.3, 0.0],
                  [0.2, 0.1, 0.1, 0.3, 0.1, 0.3, 0.0],
                  [np.nan, 0.1, 0.1, 0.3, 0.1, 0.3, 0.0]])
    truth = [0, 0, 4, 3, 1, 2]
    pred, rank, ent, tot = ar.restate(x, truth, col)
    assert pred.tolist() == [2, 2, 1, 1, 1, 2]
    assert rank[0] == 1                     # only residue 2 beats residue 0's 0.2
    assert rank[1] == 1                     # 0.3 at column 0 (residue 2) ties 0.3 at column 4 and comes first
    assert rank[2] == 3                     # residue 4's 0 is beaten by 1 (.3), 2 (.2), 0 (.1)
    assert rank[3] == ar.NEVER              # residue 3 owns no column
    assert rank[4] == 0
    assert rank[5] == 0                     # a NaN row is a hit at every k only where pred == true
    assert np.isnan(ent[5]) and not np.isnan(ent[:5]).any()
    assert tot["n_nonfinite"] == 1 and tot["rank_hist"][ar.NEVER] == 1


def test_macro_precision_recall_when_a_class_is_never_predicted():
    cm = np.zeros((20, 20), np.int64)
    cm[0, 0], cm[0, 1], cm[1, 1], cm[2, 1] = 3, 1, 2, 2         # class 2 is present but never predicted
    rank_hist = np.zeros(21, np.int64)
    rank_hist[0], rank_hist[1] = 5, 3
    m = analysis.metrics_from_totals(cm, rank_hist, 8, 0, 0, 8)
    prec = [1.0, 2 / 5] + [0.0] * 18                            # zero_division = 0 for classes never predicted
    rec = [3 / 4, 1.0, 0.0] + [0.0] * 17
    assert m["precision"] == pytest.approx(np.mean(prec), abs=1e-15)
    assert m["recall"] == pytest.approx(np.mean(rec), abs=1e-15)
    assert m["report"]["D"] == {"precision": 0.0, "recall": 0.0, "f1-score": 0.0, "support": 2}
    assert m["report"]["C"]["f1-score"] == pytest.approx(2 * 0.4 / 1.4)
    # the same through the per-row restatement
    y = np.array([0, 0, 0, 0, 1, 1, 2, 2])
    p = np.array([0, 0, 0, 1, 1, 1, 1, 1])
    r = np.array([0, 0, 0, 1, 0, 0, 1, 1])
    want = ar.metrics(y, p, r)
    assert m["precision"] == pytest.approx(want["precision"]) and m["recall"] == pytest.approx(want["recall"])
    assert m["accuracy_1"] == want["accuracy_1"] == 5 / 8 and m["accuracy_2"] == 1.0


def test_normalize_all_and_bias():
    rng = np.random.default_rng(2)
    y = rng.integers(0, 20, 500)
    p = np.where(rng.random(500) < 0.6, y, rng.integers(0, 20, 500))
    cm = np.zeros((20, 20), np.int64)
    np.add.at(cm, (y, p), 1)
    rank_hist = np.zeros(21, np.int64)
    rank_hist[0] = int(np.sum(y == p))
    rank_hist[20] = 500 - rank_hist[0]
    m = analysis.metrics_from_totals(cm, rank_hist, 500, 0, 0, 520)
    want = ar.metrics(y, p, np.where(y == p, 0, 20))
    got_cm = np.array(m["unweighted_cm"])
    assert np.allclose(got_cm, want["unweighted_cm"], rtol=0, atol=1e-15) and got_cm.sum() == pytest.approx(1.0)
    assert m["confusion_counts"] == cm.tolist()
    for c in ar.RESIDUES:
        assert m["bias"][c] == pytest.approx(want["bias"][c], abs=1e-15)
    assert sum(m["bias"].values()) == pytest.approx(0.0, abs=1e-12)
    assert m["count_labels"]["A"] == int(np.sum(y == 0)) and m["count_pred"]["Y"] == int(np.sum(p == 19))
    assert m["n_residues"] == 520 and m["n_labelled"] == 500


def test_no_labelled_rows_gives_null_metrics():
    m = analysis.metrics_from_totals(np.zeros((20, 20)), np.zeros(21), 0, 0, 0, 12, entropy=np.array([1.0, np.nan, 2.0]))
    assert m["n_labelled"] == 0 and m["accuracy_1"] is None and m["precision"] is None and m["unweighted_cm"] is None
    assert m["mean_entropy"] == 1.5


def test_blosum62_is_the_published_matrix():
    b = analysis.BLOSUM62
    assert b.shape == (20, 20) and np.array_equal(b, b.T)
    idx = {c: i for i, c in enumerate(analysis.RESIDUES)}
    diag = dict(A=4, C=9, D=6, E=5, F=6, G=6, H=8, I=4, K=5, L=4, M=5, N=6, P=7, Q=5, R=5, S=4, T=5, V=4, W=11, Y=7)
    assert {c: int(b[idx[c], idx[c]]) for c in analysis.RESIDUES} == diag
    for a, c, v in (("I", "V", 3), ("F", "Y", 3), ("K", "R", 2), ("W", "G", -2), ("D", "E", 2), ("A", "S", 1), ("W", "Y", 2),
                    ("C", "E", -4), ("L", "M", 2), ("N", "D", 1)):
        assert b[idx[a], idx[c]] == v, (a, c)


def test_column_owner_helpers():
    from design_utils import utils
    _codec, cats = utils.get_rotamer_codec()
    col = analysis.rotamer_columns(cats)
    assert col.shape == (338,) and col.dtype == np.int8
    assert np.array_equal(col, np.array([np.argmax(_codec[i]) for i in range(338)]))
    assert analysis.residue_indices(["ALA", "TYR", "UNK", "GLY"]).tolist() == [0, 19, -1, 5]
    assert analysis.identity_columns().tolist() == list(range(20))


def test_output_analysis_flag_is_documented_and_parsed():
    import predict
    help_text = dict(predict.CLI_FLAGS)["--output_analysis"]["help"]
    assert "unused" not in help_text and "_analysis.json" in help_text
    assert predict.build_parser().parse_args(["--output_analysis"]).output_analysis is True
    import inspect
    assert inspect.signature(predict.load_dataset_and_predict).parameters["output_analysis"].default is False
