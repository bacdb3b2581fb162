"""pack_sidechains.py — side chains packed by a rotamer search: for a set of PDB files, on their native backbones, the rotamer class
of every residue is CHOSEN on the GPU (th_pack_sidechains: all structures in as few submissions as the byte budget allows), built
into atoms (th_build_sidechains) and measured against the deposited side chains in Angstrom and for steric clashes.

    python pack_sidechains.py --path_to_pdb biounits/ --path_to_output packed \\
        --path_to_pred_matrix TIMED_rotamer_rot.csv --path_to_datasetmap datasetmap.txt

What the packer is: an integer steric ladder — one unit of --clash_weight for every --ladder level that two atoms of different
residues are closer than, under the pair rules of the clash count — plus, with a matrix, the model's own probabilities as
round(-1000 log2 p) over the classes of the residue's type; greedy sweeps in residue order from a deterministic start (every
residue at its best class against the backbone alone), at most --max_sweeps of them, until a sweep moves nothing.

What it is not: SCWRL4 (PARITY UNPINNED AGAINST SCWRL4: the reference packs with SCWRL4, which is not available to pin this
against and is not rebuilt), a backbone-dependent rotamer library (the candidates are the 3^n_chi classes at their bin centres,
60 / 180 / -60 degrees), hydrogen bonds or any other physics, or a global optimum.  Sterics alone is a weak packer — on 1ubq the
default ladder puts 40 of 68 chi1 bins right, with no clash left under 2.5 Angstrom — and --clash_weight 2000 (one ladder level =
two bits of probability) is a choice, not a measurement: no real model is available here to tune it against.

With a matrix, rows pair with residues through the dataset map (csv rows pdb, chain, residue number, label; one per matrix row) by
chain and residue number, as in build_sidechains.py; ``--sequence predicted`` packs the residue type of each row's arg-max class
instead of the native type (a residue without a row stays unbuilt); ``--prior none`` ignores the probabilities and packs by
sterics alone.  Without a matrix the native sequence is packed by sterics alone.

Writes ``<pdb>_<suffix>.pdb`` per structure (the suffix is ``packed_<matrix name>`` or ``packed``), ``structure_packing.csv``,
``residue_packing.csv`` (empty fields stand for absent values) and ``rotamer_labels.json`` of the packed classes, in the format
analyse_rotamers.py --path_to_rotamer_labels reads.

--lddt additionally writes ``structure_sidechain_lddt.csv`` and ``residue_sidechain_lddt.csv``: the all-atom lDDT (th_lddt_atoms) of
every packed structure against its native, residues paired by chain and number, with the names of symmetric side-chain atoms
resolved per residue.  The packer places bin centres and cannot tell the two namings of a ring or a carboxylate apart; the RMSD
columns, which stay as they are, charge it for that, ``lddt_sidechain`` does not.  The columns are those of analyse_models.py
--lddt_all_atom.  PARITY UNPINNED AGAINST OPENSTRUCTURE.
"""
import argparse
import csv
import json
import sys
from pathlib import Path

import numpy as np

from timed_hip import batching, lddt_atoms, packer, pdbio, sidechains, structure
from timed_hip.pdbio import find_structures, stem_of

STRUCTURE_COLUMNS = ["structure", "residues", "packed", "energy_initial", "energy_final", "sweeps", "moves", "converged", "status", "atoms_matched",
                     "rmsd", "clashing_pairs", "unmatched_rows"]
RESIDUE_COLUMNS = ["structure", "chain", "residue", "native", "packed", "class", "chi1", "chi2", "chi3", "chi4", "cost_initial", "cost_final",
                   "n_matched", "rmsd", "clashes"]
LABELS_FILE = "rotamer_labels.json"


def labels_of(labels, packed) -> dict:
    """{<pdb><chain>: [class or None per residue]} of the packed classes: the labels file of analyse_rotamers.py"""
    out: dict = {}
    for label, res in zip(labels, packed):
        code = stem_of(label)[:4]
        for residue, cls in zip(res.residues, res.cls.tolist()):
            out.setdefault(f"{code}{residue.chain}", []).append(None if cls < 0 else int(cls))
    return out


def write_outputs(out: Path, labels, packed, suffix: str) -> None:
    from design_utils.amino_acids import standard_amino_acids
    names = list(standard_amino_acids.values())
    out.mkdir(parents=True, exist_ok=True)
    text = lambda x: "" if x != x else repr(float(x))                       # noqa: E731
    with open(out / "structure_packing.csv", "w", newline="") as fs, open(out / "residue_packing.csv", "w", newline="") as fr:
        ws, wr = csv.writer(fs), csv.writer(fr)
        ws.writerow(STRUCTURE_COLUMNS)
        wr.writerow(RESIDUE_COLUMNS)
        for label, res in zip(labels, packed):
            built = res.built
            pdbio.write_pdb(out / f"{stem_of(label)}_{suffix}.pdb", built.to_model())
            ws.writerow([label, len(res.residues), int((res.cls >= 0).sum()), res.energy_initial, res.energy_final, res.n_sweeps, res.n_moves,
                         int(res.converged), res.status, int(built.n_matched.sum()), text(built.overall_rmsd), built.pairs, res.unmatched_rows])
            for r, native in enumerate(res.residues):
                wr.writerow([label, native.chain, native.number, native.name, names[res.res_type[r]] if res.res_type[r] >= 0 else "",
                             "" if res.cls[r] < 0 else int(res.cls[r])] + [text(x) for x in res.chi[r]] +
                            [int(res.cost_initial[r]), int(res.cost_final[r]), int(built.n_matched[r]), text(built.rmsd[r]), int(built.clashes[r])])
    with open(out / LABELS_FILE, "w") as f:
        json.dump(labels_of(labels, packed), f)
        f.write("\n")


def main(args):
    found = find_structures(args.path_to_pdb)
    if not found:
        sys.exit(f"no *.pdb / *.pdb1 / *.ent (.gz) file under {args.path_to_pdb}")
    if not args.path_to_pred_matrix and (args.sequence == "predicted" or args.prior == "matrix"):
        sys.exit("--sequence predicted and --prior matrix need --path_to_pred_matrix and --path_to_datasetmap")
    layouts = batching.parse_each(lambda item: structure.rotamer_layout(structure.first_model(item[1])), found, args.workers)
    labels = [label for label, _ in found]
    matrix = dataset_map = None
    suffix = "packed"
    if args.path_to_pred_matrix:
        from design_utils import utils as du
        from sample import _read_matrix
        matrix = _read_matrix(args.path_to_pred_matrix)
        n_classes = len(du.get_rotamer_codec()[1])
        if matrix.shape[1] != n_classes:
            raise ValueError(f"{args.path_to_pred_matrix} has {matrix.shape[1]} columns, a rotamer matrix has {n_classes}")
        dataset_map = du.load_datasetmap(Path(args.path_to_datasetmap), is_old=True)
        suffix = f"packed_{Path(args.path_to_pred_matrix).stem}"
    stats = {}
    packed = packer.pack(layouts, sequence=args.sequence, matrix=matrix, dataset_map=dataset_map, prior=args.prior, ladder=args.ladder,
                         clash_weight=args.clash_weight, max_sweeps=args.max_sweeps, clash_distance=args.clash_distance, device=args.device,
                         labels=labels, stats=stats)
    out = Path(args.path_to_output)
    write_outputs(out, labels, packed, suffix)
    if getattr(args, "lddt", False):
        scored = lddt_atoms.score_models([res.residues for res in packed], [res.built.to_model().residues for res in packed], device=args.device,
                                         stats=stats)
        lddt_atoms.write_csv(out / "structure_sidechain_lddt.csv", out / "residue_sidechain_lddt.csv",
                             [(label, path, f"{stem_of(label)}_{suffix}.pdb") for label, path in found], scored)
    atoms = sum(int(res.built.n_matched.sum()) for res in packed)
    total = float(np.sqrt(sum(float(res.built.sum_sq.sum()) for res in packed) / atoms)) if atoms else float("nan")
    print(f"{len(found)} structures, {sum(int((res.cls >= 0).sum()) for res in packed)} side chains packed ({suffix}), energy "
          f"{sum(res.energy_initial for res in packed)} -> {sum(res.energy_final for res in packed)} in at most {max(res.n_sweeps for res in packed)} sweeps "
          f"({sum(not res.converged for res in packed)} not converged, {sum(res.status != 0 for res in packed)} too long), {atoms} atoms matched, "
          f"side-chain RMSD {total:.3f} Angstrom, {sum(res.built.pairs for res in packed)} clashing pairs, "
          f"{sum(res.unmatched_rows for res in packed)} unmatched rows in {stats.get('submissions', 0)} GPU submission(s) -> {out}")
    return packed


# (flag, argparse keywords)
CLI_FLAGS = (
    ("--path_to_pdb", dict(type=str, nargs="+", default=None, required=True,
                           help="PDB files and / or directories searched for *.pdb, *.pdb1, *.ent, each optionally .gz")),
    ("--path_to_output", dict(type=str, default="packed", help="directory for the packed structures, the two csv files and rotamer_labels.json")),
    ("--path_to_pred_matrix", dict(type=str, default=None, help="338-column probability matrix written by predict.py --predict_rotamers (<model>_rot.csv)")),
    ("--path_to_datasetmap", dict(type=str, default="datasetmap.txt", help="the dataset map of the matrix (.txt): csv rows pdb, chain, residue number, label")),
    ("--sequence", dict(type=str, default="native", choices=("native", "predicted"),
                        help="pack the residue types of the structure, or those of the arg-max class of every matrix row")),
    ("--prior", dict(type=str, default=None, choices=("matrix", "none"),
                     help="add the matrix's probabilities to the energy (the default with a matrix) or pack by sterics alone")),
    ("--ladder", dict(type=float, nargs="+", default=list(packer.LADDER), help="1..8 increasing distances in Angstrom: a pair of atoms costs one unit per level it is under")),
    ("--clash_weight", dict(type=int, default=packer.CLASH_WEIGHT, help="the cost of one ladder level in units of 1/1000 bit of probability (a choice, not a measurement)")),
    ("--max_sweeps", dict(type=int, default=packer.MAX_SWEEPS, help="sweeps over the residues at most (0: the initial state)")),
    ("--clash_distance", dict(type=float, default=sidechains.CLASH_DISTANCE, help="two atoms of the result closer than this (Angstrom) are reported as a clash")),
    ("--device", dict(type=int, default=0, help="HIP device index")),
    ("--workers", dict(type=int, default=8, help="host threads that read and parse the files (at most 16)")),
    ("--lddt", dict(default=argparse.SUPPRESS, action="store_true",
                    help="also write structure_sidechain_lddt.csv and residue_sidechain_lddt.csv: the all-atom lDDT of every packed structure "
                         "against its native, symmetric side-chain names resolved.  PARITY UNPINNED AGAINST OPENSTRUCTURE")),
)


def build_parser():
    parser = argparse.ArgumentParser(description="Side chains packed by a rotamer search, RMSD to the native and clashes, batched on the GPU (MI355X)",
                                     epilog=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for flag, keywords in CLI_FLAGS:
        parser.add_argument(flag, **keywords)
    return parser


if __name__ == "__main__":
    main(build_parser().parse_args())
