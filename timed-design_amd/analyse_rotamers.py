"""analyse_rotamers.py — the reference's rotamer evaluation command line (reference analyse_rotamers.py:19-177), analysis 1: the
338-class prediction matrix of a rotamer model against the rotamers of the deposited structures, per class — ROC AUC one-vs-one
and one-vs-rest, top-1..5 accuracy, classification report, bias, plain and label-weighted confusion matrices — computed on the
GPU (design_utils.analyse_utils.calculate_rotamer_metrics -> th_analyse_classes).

    python analyse_rotamers.py --path_to_pred_matrix TIMED_rotamer_rot.csv --path_to_datasetmap datasetmap.txt \\
        --path_to_rotamer_labels rotamer_labels.json --output_path analysis

The true rotamers come from ``--path_to_rotamer_labels``: JSON {"<pdb><chain>": [class index or null, ...]}, which is the first
dict the reference's ``tag_pdb_with_rot`` returns.  With the reference installed, three lines write it:

    from design_utils.analyse_utils import tag_pdb_with_rot
    wt_results_dict, _ = tag_pdb_with_rot(workers, path_to_pdb, pdb_codes)
    json.dump({k: [None if v != v else int(v) for v in vals] for k, vals in wt_results_dict.items()}, open("rotamer_labels.json", "w"))

Tagging structures here would need ampal's side-chain dihedral code, and the reference's analyses 2 and 3 need SCWRL4; neither
can be pinned by this project's tests, so they are not rebuilt: without --path_to_rotamer_labels the program stops and says so.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

from design_utils import utils as du
from design_utils.analyse_utils import calculate_rotamer_metrics

NO_LABELS_MESSAGE = (
    "analyse_rotamers.py needs --path_to_rotamer_labels FILE: JSON {\"<pdb><chain>\": [rotamer class index or null, ...]}, the first "
    "dict the reference's tag_pdb_with_rot returns (see --help for the three lines that dump it).  Tagging the structures under "
    "--path_to_pdb needs ampal's side-chain dihedral code, and the analyses against SCWRL4-packed structures need SCWRL4 "
    "(--scwrl_path); neither is part of this build.")


def load_rotamer_labels(path) -> dict:
    with open(path) as f:
        labels = json.load(f)
    if not isinstance(labels, dict) or not all(isinstance(v, list) for v in labels.values()):
        raise ValueError(f"{path}: expected a JSON object of lists, {{\"<pdb><chain>\": [class index or null, ...]}}")
    return labels


def main(args):
    if not getattr(args, "path_to_rotamer_labels", None):
        sys.exit(NO_LABELS_MESSAGE)
    matrix_path, map_path = Path(args.path_to_pred_matrix), Path(args.path_to_datasetmap)
    labels_path = Path(args.path_to_rotamer_labels)
    model_name = matrix_path.stem
    output_path = Path(f"{args.output_path}_{model_name}")          # the reference's naming (analyse_rotamers.py:23)
    for what, path in (("prediction matrix", matrix_path), ("dataset map", map_path), ("rotamer labels file", labels_path)):
        assert path.exists(), f"No {what} at {path}"
    output_path.mkdir(parents=True, exist_ok=True)
    from sample import _one_letter_rotamer_categories, _read_matrix
    dataset_map = du.load_datasetmap(map_path, is_old=args.support_old_datasetmap)
    # float16, as the reference reads it (analyse_rotamers.py:46-48): text -> float64 -> float16 is genfromtxt's double rounding
    prediction_matrix = _read_matrix(matrix_path).astype(np.float16)
    _, flat_categories = du.get_rotamer_codec()
    if prediction_matrix.shape[1] != len(flat_categories):
        raise ValueError(f"{matrix_path} has {prediction_matrix.shape[1]} columns, a rotamer matrix has {len(flat_categories)}")
    _seq, pdb_to_probability, _real, _c, _cp = du.extract_sequence_from_pred_matrix(
        dataset_map, prediction_matrix, rotamers_categories=_one_letter_rotamer_categories(),
        old_datasetmap=args.support_old_datasetmap)
    # analysis 1 of the reference: the model against the rotamers of the deposited structure
    return calculate_rotamer_metrics(pdb_to_probability, load_rotamer_labels(labels_path), flat_categories,
                                     suffix=f"{model_name}_vs_original", output_path=output_path, device=args.device)


# (flag, argparse keywords): names, types and defaults are the reference's (analyse_rotamers.py:143-175); --path_to_rotamer_labels
# and --device are additions of this build
CLI_FLAGS = (
    ("--path_to_pred_matrix", dict(type=str, help="338-column probability matrix written by predict.py --predict_rotamers (<model>_rot.csv)")),
    ("--output_path", dict(default="output", type=str, help="the analysis is written to the directory <output_path>_<matrix name>")),
    ("--path_to_pdb", dict(type=str, help="biounit pdb dataset, pdb/{2nd and 3rd char}/{pdb}.pdb1.gz (accepted for compatibility: structures are not tagged here)")),
    ("--path_to_datasetmap", dict(default="datasetmap.txt", type=str, help="dataset map written by predict.py (.txt)")),
    ("--workers", dict(type=int, default=8, help="accepted for compatibility; the metrics are computed on the GPU")),
    ("--support_old_datasetmap", dict(default=False, action="store_true", help="the dataset map is the old 4-column csv")),
    ("--scwrl_path", dict(default="/Users/leo/scwrl4/Scwrl4", type=str, help="accepted for compatibility: the SCWRL4 analyses are not part of this build")),
    ("--path_to_rotamer_labels", dict(type=str, default=None, help="JSON {\"<pdb><chain>\": [rotamer class index or null, ...]}: the first dict tag_pdb_with_rot returns")),
    ("--device", dict(type=int, default=0, help="HIP device index")),
)


def build_parser():
    parser = argparse.ArgumentParser(description="Per-class evaluation of a rotamer prediction matrix (MI355X)",
                                     epilog=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for flag, keywords in CLI_FLAGS:
        parser.add_argument(flag, **keywords)
    return parser


if __name__ == "__main__":
    main(build_parser().parse_args())
