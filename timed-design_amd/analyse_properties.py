"""analyse_properties.py — structure properties of a set of PDB files: packing density and B-factor per residue and per structure
(reference scripts/analyse_all_properties.py, which runs design_utils.analyse_utils.extract_packdensity_from_ampal and
extract_bfactor_from_ampal over every AlphaFold2 model of every sampled sequence under a multiprocessing.Pool).  Here the files
are parsed on host threads and ALL structures go to the GPU in as few th_packing_density submissions as the byte budget allows.

    python analyse_properties.py --path_to_pdb af2_models/ extra/1ubq.pdb1.gz --path_to_output properties

Writes ``residue_properties.csv`` (structure, chain, residue number, residue name, packing density, B-factor) and
``structure_properties.csv`` (structure, atoms, residues, np.mean / np.std of the packing density and of the B-factor, and with
--path_to_pred_matrix + --path_to_datasetmap the mean and standard deviation of the prediction entropy of the structure whose
dataset-map key equals the file's stem).  The packing density is the atomic contact number within --radius, summarised per residue
by the reference's running half-average over the atoms --atom_filter_function selects; which atoms are neighbours and which
residues are reported is the structure rule of timed_hip/structure.py (first model, every non-hydrogen ATOM / HETATM atom a
neighbour, the non-hetero residues of the first chain reported; --all_chains reports every chain).  B-factor: of the residue's
first atom, as the reference reads the pLDDT of an AlphaFold2 model.

Out of scope here: the reference script's CE-align RMSD (PyMOL), which is analyse_models.py --cealign, and its parsing of AlphaFold2
file names into model / temperature / sample / rank columns — the ``structure`` column is the file's path relative to the
--path_to_pdb entry it was found under.
"""
import argparse
import csv
import sys
from pathlib import Path

import numpy as np

from timed_hip import batching, structure
from timed_hip.pdbio import PDB_SUFFIXES, find_structures, is_pdb_name, stem_of  # noqa: F401  (their home; kept importable from here)
from timed_hip.textio import float_repr as _fmt


def main(args):
    found = find_structures(args.path_to_pdb)
    if not found:
        sys.exit(f"no *.pdb / *.pdb1 / *.ent (.gz) file under {args.path_to_pdb}")
    entropy = None
    if args.path_to_pred_matrix or args.path_to_datasetmap:
        if not (args.path_to_pred_matrix and args.path_to_datasetmap):
            sys.exit("--path_to_pred_matrix and --path_to_datasetmap go together")
        from design_utils.analyse_utils import extract_prediction_entropy_to_dict
        entropy = extract_prediction_entropy_to_dict(Path(args.path_to_pred_matrix), Path(args.path_to_datasetmap),
                                                     rotamer_mode=args.rotamer_mode, is_old=args.support_old_datasetmap)

    def parse(item):
        model = structure.first_model(item[1])
        return model, structure.layout(model, args.atom_filter_function, include_hetero=True, all_chains=args.all_chains)
    parsed = batching.parse_each(parse, found, args.workers)
    stats = {}
    results = structure.packing_density_layouts([l for _, l in parsed], radius=args.radius, device=args.device,
                                                budget_bytes=int(args.batch_mb * (1 << 20)), stats=stats)
    out = Path(args.path_to_output)
    out.mkdir(parents=True, exist_ok=True)
    with open(out / "residue_properties.csv", "w", newline="") as fr, open(out / "structure_properties.csv", "w", newline="") as fs:
        wr, ws = csv.writer(fr), csv.writer(fs)
        wr.writerow(["structure", "chain", "residue_number", "residue_name", "packing_density", "bfactor"])
        head = ["structure", "atoms", "residues", "packing_density_mean", "packing_density_std", "bfactor_mean", "bfactor_std"]
        ws.writerow(head + (["entropy_mean", "entropy_std"] if entropy is not None else []))
        for (label, _), res in zip(found, results):
            bfac = np.array([float(r.bfactors.get(next(iter(r.atoms)), float("nan"))) if r.atoms else float("nan") for r in res.residues],
                            dtype=np.float64)
            for r, d, b in zip(res.residues, res.residue_density, bfac):
                wr.writerow([label, r.chain, r.number, r.name, _fmt(d), _fmt(b)])
            n = len(res.residues)
            row = [label, len(res.atom_density), n]
            for values in (res.residue_density, bfac):
                row += [_fmt(np.mean(values)), _fmt(np.std(values))] if n else ["nan", "nan"]
            if entropy is not None:
                e = entropy.get(stem_of(label))
                row += [_fmt(np.mean(e)), _fmt(np.std(e))] if e is not None and len(e) else ["nan", "nan"]
            ws.writerow(row)
    print(f"{len(found)} structures, {sum(len(r.atom_density) for r in results)} atoms, {sum(len(r.residues) for r in results)} residues "
          f"in {stats.get('submissions', 0)} GPU submission(s) -> {out}")
    return results


# (flag, argparse keywords); --path_to_pdb, --atom_filter_function and --workers are the reference script's names
CLI_FLAGS = (
    ("--path_to_pdb", dict(type=str, nargs="+", default=None, required=True,
                           help="PDB files and / or directories searched for *.pdb, *.pdb1, *.ent, each optionally .gz")),
    ("--atom_filter_function", dict(type=str, default="all", choices=["all", "ca", "backbone", "calpha"],
                                    help="atoms of a residue that enter its packing density: all (default, as the reference script), "
                                         "ca (the reference's substring test: atoms named C and CA), backbone (N CA C O), calpha (CA alone)")),
    ("--radius", dict(type=float, default=7.0, help="contact radius in Angstrom (default 7, Weiss 2007)")),
    ("--path_to_output", dict(type=str, default="properties", help="directory for residue_properties.csv and structure_properties.csv")),
    ("--workers", dict(type=int, default=8, help="host threads that read and parse the files (at most 16)")),
    ("--device", dict(type=int, default=0, help="HIP device index")),
    ("--all_chains", dict(default=False, action="store_true", help="report the residues of every chain, not only the first")),
    ("--batch_mb", dict(type=float, default=256.0, help="atom-array megabytes per GPU submission (default 256)")),
    ("--path_to_pred_matrix", dict(type=str, default=None, help="prediction matrix CSV (predict.py): adds entropy_mean / entropy_std per structure")),
    ("--path_to_datasetmap", dict(type=str, default=None, help="its dataset map; a structure is matched by its file stem")),
    ("--rotamer_mode", dict(default=False, action="store_true", help="the prediction matrix has 338 columns")),
    ("--support_old_datasetmap", dict(default=False, action="store_true", help="the dataset map is the old 4-column csv")),
)


def build_parser():
    parser = argparse.ArgumentParser(description="Packing density and B-factor of PDB structures, batched on the GPU (MI355X)",
                                     epilog=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for flag, keywords in CLI_FLAGS:
        parser.add_argument(flag, **keywords)
    return parser


if __name__ == "__main__":
    main(build_parser().parse_args())
