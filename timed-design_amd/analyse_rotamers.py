"""analyse_rotamers.py — the reference's rotamer evaluation command line (reference analyse_rotamers.py:19-177), analysis 1: the
338-class prediction matrix of a rotamer model against the rotamers of the deposited structures, per class — ROC AUC one-vs-one
and one-vs-rest, top-1..5 accuracy, classification report, bias, plain and label-weighted confusion matrices — computed on the
GPU (design_utils.analyse_utils.calculate_rotamer_metrics -> th_analyse_classes).

    python analyse_rotamers.py --path_to_pred_matrix TIMED_rotamer_rot.csv --path_to_datasetmap datasetmap.txt \\
        --path_to_rotamer_labels rotamer_labels.json --output_path analysis

The true rotamers come from ``--path_to_rotamer_labels``: JSON {"<pdb><chain>": [class index or null, ...]}, which is the first
dict the reference's ``tag_pdb_with_rot`` returns, or — without that flag — from the structures under ``--path_to_pdb``:

    python analyse_rotamers.py --path_to_pred_matrix TIMED_rotamer_rot.csv --path_to_datasetmap datasetmap.txt \\
        --path_to_pdb biounits/ --output_path analysis

tags the structures of the dataset map's pdb codes here (design_utils.analyse_utils.tag_pdb_with_rot: the reference's file rule,
``<path>/<code[1:3]>/<code[:4]>.pdb1.gz`` then ``.pdb1``, ``<path>/<code>.pdb`` for a code with ``_``; nothing is fetched; chi
angles and classes on the GPU, th_tag_rotamers), writes ``rotamer_labels.json`` into the output directory in the format above, and
runs the analysis on it.  The reference tags with ampal's side-chain dihedral code, which is not available to pin this against:
the atom paths, bin edges and the ALA / GLY class are this project's own rule, written out in timed_hip/structure.py (PARITY
UNPINNED AGAINST AMPAL).  Labels and matrix rows are paired by position, as the reference pairs them.  ``tag_rotamers.py`` writes
the same labels file (and the chi angles) for any set of PDB files.

The reference's analyses 2 and 3 hand a sequence and the backbone to SCWRL4, tag the packed structure again and score the model
against it.  SCWRL4 is not available to pin anything against and is not rebuilt; ``--pack`` (with --path_to_pdb) runs both analyses
in process with this project's own packer instead (timed_hip.packer: an integer steric ladder, greedy sweeps from a deterministic
start — PARITY UNPINNED AGAINST SCWRL4, it is neither SCWRL4's rotamer library nor its energy).  The predicted sequence and the
native sequence are each packed onto the native backbones WITHOUT the model's probabilities, so that the packer is as independent
of the model it is compared with as SCWRL4 is; the packed structures (``<pdb>_packed_<model>.pdb``, ``<pdb>_wt_packed.pdb``) are
tagged again and ``results_<model>_vs_packed_<model>`` and ``results_<model>_vs_wt_packed`` (.txt, .json, confusion csv files) are
written like analysis 1, with ``packing_scores.csv`` (PDB,score_rot,score_real: the packer's final energies) where the reference
writes scwrl_scores.csv.  Without --pack the program writes what it always wrote.

With neither --path_to_rotamer_labels nor --path_to_pdb the program stops and says so.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

from design_utils import utils as du
from design_utils.analyse_utils import calculate_rotamer_metrics

NO_LABELS_MESSAGE = (
    "analyse_rotamers.py needs the true rotamers: either --path_to_rotamer_labels FILE, JSON {\"<pdb><chain>\": [rotamer class index "
    "or null, ...]} — the first dict the reference's tag_pdb_with_rot returns, or what tag_rotamers.py writes — or --path_to_pdb DIR, "
    "the biounit structures of the dataset map's pdb codes, which are then tagged here (this project's own rule: ampal's side-chain "
    "dihedral code is not available to pin it).  The analyses against SCWRL4-packed structures need SCWRL4 (--scwrl_path) and are "
    "not part of this build.")
LABELS_FILE = "rotamer_labels.json"
SCORES_FILE = "packing_scores.csv"


def load_rotamer_labels(path) -> dict:
    with open(path) as f:
        labels = json.load(f)
    if not isinstance(labels, dict) or not all(isinstance(v, list) for v in labels.values()):
        raise ValueError(f"{path}: expected a JSON object of lists, {{\"<pdb><chain>\": [class index or null, ...]}}")
    return labels


def tag_structures(args, dataset_map, output_path: Path) -> Path:
    """tag the structures of the map's pdb codes under --path_to_pdb and write the labels file into the output directory"""
    from design_utils.analyse_utils import rotamer_labels_json, tag_pdb_with_rot
    pdb_codes = np.unique(np.asarray([row[0] for row in dataset_map]))           # as the reference (analyse_rotamers.py:41)
    wt_results_dict, _assemblies = tag_pdb_with_rot(args.workers, Path(args.path_to_pdb), pdb_codes, device=args.device)
    labels_path = output_path / LABELS_FILE
    with open(labels_path, "w") as f:
        json.dump(rotamer_labels_json(wt_results_dict), f)
        f.write("\n")
    print(f"tagged {len(wt_results_dict)} chains of {len(pdb_codes)} pdb codes -> {labels_path}")
    return labels_path


def analyse_packed(args, dataset_map, pdb_to_sequence, pdb_to_probability, flat_categories, model_name: str, output_path: Path) -> dict:
    """analyses 2 and 3 of the reference with this project's packer in SCWRL4's place: {suffix: metrics}"""
    from design_utils.analyse_utils import analyse_with_packer, tag_pdb_with_rot
    pdb_codes = np.unique(np.asarray([str(row[0])[:4] for row in dataset_map]))
    _, pdb_to_assemblies = tag_pdb_with_rot(args.workers, Path(args.path_to_pdb), pdb_codes, device=args.device)
    real = {f"{code}{chain_id}": chain.sequence for code, chains in pdb_to_assemblies.items() for chain_id, chain in chains.items()}
    results, scores = {}, {}
    for column, sequences, file_suffix, result_suffix in (
            ("score_rot", pdb_to_sequence, f"_packed_{model_name}", f"{model_name}_vs_packed_{model_name}"),
            ("score_real", {key: real[key] for key in pdb_to_sequence if key in real}, "_wt_packed", f"{model_name}_vs_wt_packed")):
        scores[column], packed = analyse_with_packer(sequences, pdb_to_assemblies, output_path, suffix=file_suffix, device=args.device)
        packed_labels, _ = tag_pdb_with_rot(args.workers, output_path, [code + file_suffix for code in packed], device=args.device)
        results[result_suffix] = calculate_rotamer_metrics(pdb_to_probability, packed_labels, flat_categories, suffix=result_suffix,
                                                           output_path=output_path, device=args.device)
    with open(output_path / SCORES_FILE, "w") as f:
        f.write("PDB,score_rot,score_real\n")
        for pdb, score_rot in scores["score_rot"].items():
            f.write(f"{pdb},{score_rot},{scores['score_real'].get(pdb, '')}\n")
    return results


def main(args):
    labels_given = getattr(args, "path_to_rotamer_labels", None)
    if not labels_given and not getattr(args, "path_to_pdb", None):
        sys.exit(NO_LABELS_MESSAGE)
    pack = getattr(args, "pack", False)
    if pack and not getattr(args, "path_to_pdb", None):
        sys.exit("--pack packs the structures of the dataset map's pdb codes: it needs --path_to_pdb DIR")
    matrix_path, map_path = Path(args.path_to_pred_matrix), Path(args.path_to_datasetmap)
    model_name = matrix_path.stem
    output_path = Path(f"{args.output_path}_{model_name}")          # the reference's naming (analyse_rotamers.py:23)
    checks = [("prediction matrix", matrix_path), ("dataset map", map_path)]
    checks.append(("rotamer labels file", Path(labels_given)) if labels_given else ("PDB folder", Path(args.path_to_pdb)))
    for what, path in checks:
        assert path.exists(), f"No {what} at {path}"
    output_path.mkdir(parents=True, exist_ok=True)
    from sample import _one_letter_rotamer_categories, _read_matrix
    dataset_map = du.load_datasetmap(map_path, is_old=args.support_old_datasetmap)
    labels_path = Path(labels_given) if labels_given else tag_structures(args, dataset_map, output_path)
    # float16, as the reference reads it (analyse_rotamers.py:46-48): text -> float64 -> float16 is genfromtxt's double rounding
    prediction_matrix = _read_matrix(matrix_path).astype(np.float16)
    _, flat_categories = du.get_rotamer_codec()
    if prediction_matrix.shape[1] != len(flat_categories):
        raise ValueError(f"{matrix_path} has {prediction_matrix.shape[1]} columns, a rotamer matrix has {len(flat_categories)}")
    pdb_to_sequence, pdb_to_probability, _real, _c, _cp = du.extract_sequence_from_pred_matrix(
        dataset_map, prediction_matrix, rotamers_categories=_one_letter_rotamer_categories(),
        old_datasetmap=args.support_old_datasetmap)
    # analysis 1 of the reference: the model against the rotamers of the deposited structure
    results = calculate_rotamer_metrics(pdb_to_probability, load_rotamer_labels(labels_path), flat_categories,
                                        suffix=f"{model_name}_vs_original", output_path=output_path, device=args.device)
    if pack:
        # analyses 2 and 3 of the reference, this project's packer in SCWRL4's place
        analyse_packed(args, dataset_map, pdb_to_sequence, pdb_to_probability, flat_categories, model_name, output_path)
    return results


# (flag, argparse keywords): names, types and defaults are the reference's (analyse_rotamers.py:143-175); --path_to_rotamer_labels
# --pack and --device are additions of this build
CLI_FLAGS = (
    ("--path_to_pred_matrix", dict(type=str, help="338-column probability matrix written by predict.py --predict_rotamers (<model>_rot.csv)")),
    ("--output_path", dict(default="output", type=str, help="the analysis is written to the directory <output_path>_<matrix name>")),
    ("--path_to_pdb", dict(type=str, help="biounit pdb dataset, pdb/{2nd and 3rd char}/{pdb}.pdb1.gz: without --path_to_rotamer_labels its structures are tagged here and rotamer_labels.json is written")),
    ("--path_to_datasetmap", dict(default="datasetmap.txt", type=str, help="dataset map written by predict.py (.txt)")),
    ("--workers", dict(type=int, default=8, help="host threads that parse the structures of --path_to_pdb (at most 16); the metrics are computed on the GPU")),
    ("--support_old_datasetmap", dict(default=False, action="store_true", help="the dataset map is the old 4-column csv")),
    ("--scwrl_path", dict(default="/Users/leo/scwrl4/Scwrl4", type=str, help="accepted for compatibility: SCWRL4 is never called (--pack runs those analyses with this project's own packer); build_sidechains.py builds the predicted classes into side chains and measures them against the native (RMSD, clashes) without SCWRL4")),
    # absent from the namespace unless given (main reads it with getattr): the flags and defaults above stay the reference's set
    ("--pack", dict(default=argparse.SUPPRESS, action="store_true", help="with --path_to_pdb: also run the reference's analyses 2 and 3 with this project's own side-chain packer in SCWRL4's place (PARITY UNPINNED AGAINST SCWRL4) and write packing_scores.csv")),
    ("--path_to_rotamer_labels", dict(type=str, default=None, help="JSON {\"<pdb><chain>\": [rotamer class index or null, ...]}: the first dict tag_pdb_with_rot returns (tag_rotamers.py writes it)")),
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
