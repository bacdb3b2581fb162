"""Per-class evaluation without a GPU: the NumPy restatement of th_analyse_classes (tests/class_analysis_restatement.py) fed to
roc_auc_from_pairs / class_metrics_from_totals against the sklearn fixture (tests/golden/class_auc_golden.npz) at 1e-9 and, where
scikit-learn is installed, against sklearn itself; the None rules; the weighted confusion formula; calculate_rotamer_metrics'
pairing rules; the command-line surface of analyse_rotamers.py and predict.py --output_auc."""
import inspect
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import class_analysis_restatement as cr  # noqa: E402
from timed_hip import analysis  # noqa: E402

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-9


def _metrics(x, y, categories=None):
    r = cr.restate(x, y)
    return r, analysis.class_metrics_from_totals(r["confusion"], r["rank_hist"], r["scored_count"], r["pair_u2"], r["n_labelled"],
                                                 r["n_nonfinite"], r["n_scored"], x.shape[0], categories)


def _fixture_case(name):
    z = np.load(os.path.join(G, "class_auc_golden.npz"))
    x, y = cr.golden_matrix(name)
    assert cr.matrix_sha256(x) == str(z[f"{name}_sha256"]) and np.array_equal(y, z[f"{name}_labels"])
    return z, x, y


def test_fixture_is_small_and_its_float32_rows_are_exact():
    assert os.path.getsize(os.path.join(G, "class_auc_golden.npz")) < 64 * 1024
    for name in ("a", "b", "c"):
        x, y = cr.golden_matrix(name)
        assert x.dtype == np.float32 and np.all(x.astype(np.float64).sum(axis=1) == 1.0)
        own = x[np.arange(len(y)), y]
        assert np.all((x == own[:, None]).sum(axis=1) == 1)     # no true class tied within its row: top-k comparable
        # exact ties BETWEEN rows of different classes exist in the columns (the tie term of the AUC)
        r = cr.restate(x, y)
        assert (r["pair_u2"] % 2 == 1).any()


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_float32_cases_against_the_sklearn_fixture(name):
    z, x, y = _fixture_case(name)
    k = x.shape[1]
    r, m = _metrics(x, y)
    assert abs(m["auc_ovo"] - float(z[f"{name}_auc_ovo"])) <= TOL
    if np.isnan(z[f"{name}_auc_ovr"]):
        assert name == "c" and m["auc_ovr"] is None and m["auc_ovr_present"] is not None and m["n_classes_present"] == 200
        assert [v is None for v in m["auc_ovr_per_class"]] == [c >= 200 for c in range(k)]
    else:
        assert abs(m["auc_ovr"] - float(z[f"{name}_auc_ovr"])) <= TOL and m["auc_ovr"] == m["auc_ovr_present"]
    for kk in range(1, 6):
        assert abs(m[f"accuracy_{kk}"] - float(z[f"{name}_top_k"][kk - 1])) <= TOL
    assert 0.05 < m["accuracy_1"] < 0.95
    assert abs(m["precision"] - float(z[f"{name}_precision"])) <= TOL and abs(m["recall"] - float(z[f"{name}_recall"])) <= TOL
    assert np.array_equal(r["confusion"], z[f"{name}_cm"])
    nz = z[f"{name}_cm_nonzero"]
    for key in ("unweighted", "weighted"):
        want = np.zeros(k * k)
        want[nz] = z[f"{name}_cm_{key}"]
        assert np.abs(np.array(m[f"{key}_cm"]).ravel() - want).max() <= TOL, key
    json.dumps(m, allow_nan=False)


def test_float16_case_against_the_sklearn_fixture():
    z, x, y = _fixture_case("d")
    assert x.dtype == np.float16 and not np.allclose(1, x.astype(np.float64).sum(axis=1), atol=1e-8, rtol=0)
    r, m = _metrics(x, y)
    col = x[:, 5]
    assert np.unique(col).size < 0.95 * col.size                # float16 columns hold many exact ties
    assert abs(m["auc_ovo"] - float(z["d_auc_ovo"])) <= TOL
    assert np.abs(np.array(m["auc_ovr_per_class"], dtype=np.float64) - z["d_ovr_per_class"]).max() <= TOL
    cnt = r["scored_count"].astype(np.float64)
    a, b = z["d_pairs"][:, 0].astype(int), z["d_pairs"][:, 1].astype(int)
    assert np.abs(r["pair_u2"][a, b] / (2.0 * cnt[a] * cnt[b]) - z["d_pair_auc"]).max() <= TOL


def test_against_live_sklearn():
    sk = pytest.importorskip("sklearn.metrics")
    rs = np.random.RandomState(3)
    n, k = 600, 12
    counts = rs.randint(0, 64, (n, k)).astype(np.float64) + 1   # few distinct values: many ties
    y = rs.randint(0, k, n)
    counts[np.arange(n), y] += rs.randint(0, 64, n)
    x = counts / counts.sum(axis=1, keepdims=True)
    x32 = x.astype(np.float32)
    x64 = x32.astype(np.float64)
    r, m = _metrics(x32, y)
    for c in range(k):
        assert abs(m["auc_ovr_per_class"][c] - sk.roc_auc_score(y == c, x64[:, c])) <= TOL
    pair = 0.0
    for a in range(k):
        for b in range(a + 1, k):
            rows = np.flatnonzero((y == a) | (y == b))
            pair += (sk.roc_auc_score(y[rows] == a, x64[rows, a]) + sk.roc_auc_score(y[rows] == b, x64[rows, b])) / 2
    assert abs(m["auc_ovo"] - pair / (k * (k - 1) / 2)) <= TOL
    pred = np.argmax(x32, axis=1)
    assert np.array_equal(r["confusion"], sk.confusion_matrix(y, pred, labels=list(range(k))))
    w = np.bincount(y, minlength=k)[y] / float(n)
    want = sk.confusion_matrix(y, pred, labels=list(range(k)), normalize="all", sample_weight=w)
    assert np.abs(np.array(m["weighted_cm"]) - want).max() <= TOL


def test_u2_by_brute_force_with_ties_zeros_and_non_finite_rows():
    x = np.array([[0.5, 0.5, 0.0],
                  [0.5, 0.25, -0.0],
                  [0.25, 0.5, 0.0],
                  [0.5, 0.0, np.nan],         # not scored, predicted 2 (the NaN) != its label: rank k
                  [0.125, 0.125, 0.75],
                  [np.inf, 0.0, 0.0],         # not scored, predicted 0 = its label: rank 0
                  [0.0, 1.0, -1.0],
                  [0.3, 0.3, 0.4]], dtype=np.float32)
    y = np.array([0, 0, 1, 1, 2, 0, 2, -1])
    r = cr.restate(x, y)
    assert (r["n_labelled"], r["n_nonfinite"], r["n_scored"]) == (7, 2, 5)
    assert r["scored_count"].tolist() == [2, 1, 2]
    assert r["rank"].tolist() == [0, 0, 0, 3, 0, 0, 2, -1] and r["pred"].tolist() == [0, 0, 1, 2, 2, 0, 1, 2]
    scored = [0, 1, 2, 4, 6]
    want = np.zeros((3, 3), np.int64)
    for i in scored:
        for j in scored:
            a, b = y[i], y[j]
            if a != b:
                want[a, b] += 2 * (x[i, a] > x[j, a]) + (x[i, a] == x[j, a])
    assert np.array_equal(r["pair_u2"], want)
    assert want[2, 0] == 2 + 2 + 0 + 0                       # 0.75 beats the 0.0 and the -0.0 of class 0 (2 + 2); -1.0 loses to both
    auc = analysis.roc_auc_from_pairs(r["pair_u2"], r["scored_count"])
    assert auc["auc_ovr_per_class"][0] == (want[0, 1] + want[0, 2]) / (2.0 * 2 * 3)


def test_none_rules():
    k = 5
    u2 = np.zeros((k, k), np.int64)
    none = analysis.roc_auc_from_pairs(u2, np.zeros(k, np.int64))                # no scored row
    assert none == {"n_classes_present": 0, "auc_ovo": None, "auc_ovr_per_class": [None] * k, "auc_ovr": None,
                    "auc_ovr_present": None}
    one = analysis.roc_auc_from_pairs(u2, np.array([0, 9, 0, 0, 0]))              # one class holds every row
    assert one["auc_ovo"] is None and one["auc_ovr"] is None and one["auc_ovr_present"] is None and one["n_classes_present"] == 1
    u2[1, 3], u2[3, 1] = 2 * 6, 0                                                 # class 1 always above class 3
    two = analysis.roc_auc_from_pairs(u2, np.array([0, 2, 0, 3, 0]))
    assert two["auc_ovo"] == 0.5 and two["auc_ovr"] is None and two["auc_ovr_per_class"] == [None, 1.0, None, 0.0, None]
    assert two["auc_ovr_present"] == 0.5 and two["n_classes_present"] == 2
    # no labelled row: every metric None, JSON-safe
    x = np.full((3, 4), 0.25, np.float32)
    _, m = _metrics(x, np.full(3, -1))
    for key in ("accuracy_1", "accuracy_5", "precision", "recall", "report", "bias", "unweighted_cm", "weighted_cm", "auc_ovo", "auc_ovr"):
        assert m[key] is None, key
    assert m["n_rows"] == 3 and m["n_labelled"] == 0
    json.dumps(m, allow_nan=False)
    # a class that is never predicted has no bias (the reference writes NaN), precision 0
    x = np.array([[0.6, 0.3, 0.1], [0.5, 0.4, 0.1], [0.2, 0.7, 0.1]], np.float32)
    _, m = _metrics(x, np.array([0, 2, 1]), categories=["A_1", "B_1", "C_1"])
    assert m["bias"]["C_1"] is None and m["bias"]["A_1"] == 2 / 3 - 1 / 3 and m["report"]["C_1"]["precision"] == 0.0
    assert m["count_labels"] == {"A_1": 1, "B_1": 1, "C_1": 1} and m["count_pred"] == {"A_1": 2, "B_1": 1, "C_1": 0}
    assert m["accuracy_1"] == 2 / 3 and m["accuracy_2"] == 2 / 3 and m["accuracy_3"] == 1.0


def test_weighted_confusion_formula():
    cm = np.array([[3, 1, 0], [0, 2, 2], [0, 0, 0]])
    labels = cm.sum(axis=1)
    # sample_weight = count[y] / N, normalize="all": every row of class t weighs n_t / N, the total weight is sum n_t^2 / N
    n = labels.sum()
    weights = cm * (labels[:, None] / n)
    want = weights / weights.sum()
    got = analysis.weighted_confusion(cm)
    assert np.abs(got - want).max() < 1e-15 and abs(got.sum() - 1) < 1e-15
    assert analysis.weighted_confusion(np.zeros((3, 3), np.int64)) is None


def _restated_analyse_classes(matrix, true_class, device=0, auc=True, rows=True):
    r = cr.restate(np.asarray(matrix), true_class, auc=auc)
    return analysis.ClassAnalysis(r["pred"] if rows else None, r["rank"] if rows else None, r["confusion"], r["rank_hist"],
                                  r["scored_count"], r["pair_u2"], r["n_labelled"], r["n_nonfinite"], r["n_scored"])


def test_calculate_rotamer_metrics_pairing_rules(monkeypatch, tmp_path, capsys):
    from design_utils import analyse_utils as au
    monkeypatch.setattr(analysis, "analyse_classes", _restated_analyse_classes)
    k = 6
    cats = [f"RES_{i}" for i in range(k)]
    rng = np.random.default_rng(1)
    x = rng.dirichlet(np.ones(k), 12).astype(np.float16)
    probs = {"1abcA": x[:5].tolist(), "2defB": x[5:8].tolist(), "3ghiC": x[8:10].tolist(), "4jklD": x[10:].tolist()}
    rot = {"1abcA": [0, 1, np.nan, 3, 4], "2defB": [1, 2], "4jklD": [None, 5], "9zzzZ": [0]}
    res = au.calculate_rotamer_metrics(probs, rot, cats, "t", tmp_path)
    said = capsys.readouterr().out
    assert "Error with pdb code 2defB - Length Mismatch" in said and "Error with pdb code 3ghiC\n" in said
    assert "1abcA" not in said and "4jklD" not in said
    rows = np.concatenate([x[:5], x[10:]])
    truth = np.array([0, 1, -1, 3, 4, -1, 5])
    _, want = _metrics(rows, truth, cats)
    assert res == want and res["n_rows"] == 7 and res["n_labelled"] == 5
    assert json.loads((tmp_path / "results_t.json").read_text()) == json.loads(json.dumps(want))
    text = (tmp_path / "results_t.txt").read_text()
    for label in ("Metrics AUC_OVR:", "Metrics AUC_OVO:", "Accuracy:", "accuracy_2:", "accuracy_3:", "accuracy_4:", "accuracy_5:",
                  "precision:", "recall:", "Report:", "Bias:"):
        assert label in text, label
    for kind in ("unweighted", "weighted"):
        assert np.array_equal(np.loadtxt(tmp_path / f"cm_t_{kind}.csv", delimiter=","), np.array(want[f"{kind}_cm"]))


def test_analyse_rotamers_parser_carries_the_reference_flags_and_defaults():
    import analyse_rotamers
    args = analyse_rotamers.build_parser().parse_args([])
    assert vars(args) == {"path_to_pred_matrix": None, "output_path": "output", "path_to_pdb": None,
                          "path_to_datasetmap": "datasetmap.txt", "workers": 8, "support_old_datasetmap": False,
                          "scwrl_path": "/Users/leo/scwrl4/Scwrl4", "path_to_rotamer_labels": None, "device": 0}
    args = analyse_rotamers.build_parser().parse_args(["--support_old_datasetmap", "--workers", "3", "--path_to_pdb", "p"])
    assert args.support_old_datasetmap is True and args.workers == 3 and args.path_to_pdb == "p"


def test_analyse_rotamers_without_a_labels_file_says_what_is_missing(tmp_path):
    import analyse_rotamers
    args = analyse_rotamers.build_parser().parse_args(["--path_to_pred_matrix", str(tmp_path / "M_rot.csv")])
    with pytest.raises(SystemExit) as stop:
        analyse_rotamers.main(args)
    msg = str(stop.value)
    for word in ("--path_to_rotamer_labels", "tag_pdb_with_rot", "ampal", "SCWRL4"):
        assert word in msg, word
    assert not list(tmp_path.iterdir())


def test_output_auc_flag_and_keyword():
    import predict
    assert predict.build_parser().parse_args([]).output_auc is False
    assert predict.build_parser().parse_args(["--output_auc"]).output_auc is True
    assert inspect.signature(predict.load_dataset_and_predict).parameters["output_auc"].default is False
    with pytest.raises(ValueError, match="analyse_rotamers.py"):
        predict.load_dataset_and_predict([], "none.hdf5", predict_rotamers=True, output_auc=True)
