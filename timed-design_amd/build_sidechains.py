"""build_sidechains.py — full-atom structures from rotamer classes: the side chains of a set of PDB files built on their native
backbones from the classes a rotamer model predicts (or from the native classes or angles), measured against the deposited side
chains in Angstrom and for steric clashes, on the GPU for all structures in as few th_build_sidechains submissions as the byte
budget allows.  This is where a row of ``<model>_rot.csv`` becomes atoms.

    python build_sidechains.py --path_to_pdb biounits/ --path_to_output built \\
        --path_to_pred_matrix TIMED_rotamer_rot.csv --path_to_datasetmap datasetmap.txt

With a matrix, the arg-max class (the first maximum) of every row is built at the centres of its bins (60 / 180 / -60 degrees), as
the residue the class names: a predicted mutation is built as the predicted residue.  Rows pair with residues through the dataset
map, which must be the csv map with one (pdb, chain, residue number, label) row per matrix row: by chain and residue number,
insertion code included — the rule of ``timed_hip.structure.labels_for_map``; a "<pdb><chain> <count>" map names no residues and
is refused.  A structure takes the rows whose pdb code equals the first four characters of its file name.  A row without a
residue is counted in ``unmatched_rows`` and reported, not guessed; a residue without a row is left unbuilt.

Without a matrix, the structure's own rotamers are rebuilt: ``--chi class_centres`` (default) builds the native classes at their
bin centres — what the three-bin discretisation costs by itself, the floor under any model's number —, ``--chi native`` builds
the native angles, which leaves the error of the table alone.

Writes ``<pdb>_<suffix>.pdb`` per structure (N, CA, C, O of the native with their B-factors, the built side chains with B-factor
0.00; the suffix is the matrix's name, ``native_classes`` or ``native_chi``), ``structure_sidechains.csv`` (structure, residues,
built, native_type — built residues of the native's type —, atoms_matched, rmsd, clashing_pairs, unmatched_rows) and
``residue_sidechains.csv`` (structure, chain, residue, native, built, class, chi1..chi4 as used, n_built, n_matched, rmsd,
clashes; empty fields stand for absent values).

PARITY UNPINNED AGAINST SCWRL4: the reference packs side chains with SCWRL4's energy search, which is not available to pin this
against and is not rebuilt.  The table of internal coordinates and the rules (atoms paired by name without symmetry correction;
a clash is a side-chain atom within --clash_distance of an atom of another residue, the backbone of chain neighbours and SG-SG
excepted) are this project's own, written out in timed_hip/sidechains.py.

--lddt additionally writes ``structure_sidechain_lddt.csv`` and ``residue_sidechain_lddt.csv``: the all-atom lDDT (th_lddt_atoms) of
every built structure against its native, residues paired by chain and number, with the names of symmetric side-chain atoms
resolved per residue — the symmetry-aware companion of the RMSD columns, which stay as they are.  The columns are those of
analyse_models.py --lddt_all_atom; ``lddt_sidechain`` is the figure for the built atoms, a side chain that was not built counts as
missing.  PARITY UNPINNED AGAINST OPENSTRUCTURE.
"""
import argparse
import csv
import sys
from pathlib import Path

import numpy as np

from timed_hip import batching, lddt_atoms, pdbio, sidechains, structure
from timed_hip.pdbio import find_structures, stem_of

STRUCTURE_COLUMNS = ["structure", "residues", "built", "native_type", "atoms_matched", "rmsd", "clashing_pairs", "unmatched_rows"]
RESIDUE_COLUMNS = ["structure", "chain", "residue", "native", "built", "class", "chi1", "chi2", "chi3", "chi4", "n_built", "n_matched",
                   "rmsd", "clashes"]


def classes_from_matrix(matrix: np.ndarray, map_rows, labels, layouts):
    """per structure (int16 classes, -1 where no row names the residue; rows of the map without a residue): matrix row k belongs
    to map row k = (pdb, chain, residue number, label), and to the first residue of that chain and number in the structure whose
    file name starts with the pdb code"""
    if len(map_rows) != len(matrix) or any(len(row) < 4 for row in map_rows):
        raise ValueError(f"the dataset map has {len(map_rows)} rows for {len(matrix)} matrix rows; it must be the csv map with one "
                         "(pdb, chain, residue number, label) row per matrix row: residues are paired by chain and number")
    chosen = np.argmax(matrix, axis=1)
    per_code: dict = {}
    for k, row in enumerate(map_rows):
        per_code.setdefault(str(row[0])[:4].lower(), []).append((str(row[1]).strip(), str(row[2]).strip(), k))
    out = []
    for label, layout in zip(labels, layouts):
        cls = np.full(len(layout.residues), -1, np.int16)
        unmatched = 0
        by_key = {}
        for r, res in enumerate(layout.residues):
            by_key.setdefault((res.chain, res.number), r)
        for chain, number, k in per_code.get(stem_of(label)[:4].lower(), []):
            if (chain, number) in by_key:
                cls[by_key[(chain, number)]] = chosen[k]
            else:
                unmatched += 1
        out.append((cls, unmatched))
    return out


def main(args):
    found = find_structures(args.path_to_pdb)
    if not found:
        sys.exit(f"no *.pdb / *.pdb1 / *.ent (.gz) file under {args.path_to_pdb}")
    if args.path_to_pred_matrix and args.chi == "native":
        sys.exit("--chi native rebuilds the structure's own angles; a prediction matrix is built at its class centres")
    layouts = batching.parse_each(lambda item: structure.rotamer_layout(structure.first_model(item[1])), found, args.workers)
    labels = [label for label, _ in found]
    stats = {}
    if args.path_to_pred_matrix:
        from design_utils import utils as du
        from sample import _read_matrix
        matrix = _read_matrix(args.path_to_pred_matrix)
        n_classes = len(du.get_rotamer_codec()[1])
        if matrix.shape[1] != n_classes:
            raise ValueError(f"{args.path_to_pred_matrix} has {matrix.shape[1]} columns, a rotamer matrix has {n_classes}")
        paired = classes_from_matrix(matrix, du.load_datasetmap(Path(args.path_to_datasetmap), is_old=True), labels, layouts)
        suffix = Path(args.path_to_pred_matrix).stem
        built = sidechains.build(layouts, chi="class_centres", classes=[cls for cls, _ in paired], clash_distance=args.clash_distance,
                                 device=args.device, stats=stats)
        unmatched = [n for _, n in paired]
    else:
        suffix = "native_chi" if args.chi == "native" else "native_classes"
        built = sidechains.build(layouts, chi=args.chi, clash_distance=args.clash_distance, device=args.device, stats=stats)
        unmatched = [0] * len(built)
    out = Path(args.path_to_output)
    out.mkdir(parents=True, exist_ok=True)
    text = lambda x: "" if x != x else repr(float(x))                       # noqa: E731
    with open(out / "structure_sidechains.csv", "w", newline="") as fs, open(out / "residue_sidechains.csv", "w", newline="") as fr:
        ws, wr = csv.writer(fs), csv.writer(fr)
        ws.writerow(STRUCTURE_COLUMNS)
        wr.writerow(RESIDUE_COLUMNS)
        for label, res, missing in zip(labels, built, unmatched):
            pdbio.write_pdb(out / f"{stem_of(label)}_{suffix}.pdb", res.to_model())
            same = [b == r.name for b, r in zip(res.built_names, res.residues)]
            ws.writerow([label, len(res.residues), int((res.n_built > 0).sum()), int(((res.n_built > 0) & np.array(same, dtype=bool)).sum()),
                         int(res.n_matched.sum()), text(res.overall_rmsd), res.pairs, missing])
            for r, native in enumerate(res.residues):
                wr.writerow([label, native.chain, native.number, native.name, res.built_names[r] or "",
                             "" if res.cls is None or res.cls[r] < 0 else int(res.cls[r])] + [text(x) for x in res.chi[r]] +
                            [int(res.n_built[r]), int(res.n_matched[r]), text(res.rmsd[r]), int(res.clashes[r])])
    if getattr(args, "lddt", False):
        scored = lddt_atoms.score_models([res.residues for res in built], [res.to_model().residues for res in built], device=args.device, stats=stats)
        lddt_atoms.write_csv(out / "structure_sidechain_lddt.csv", out / "residue_sidechain_lddt.csv",
                             [(label, path, f"{stem_of(label)}_{suffix}.pdb") for label, path in found], scored)
    atoms = sum(int(res.n_matched.sum()) for res in built)
    total = float(np.sqrt(sum(float(res.sum_sq.sum()) for res in built) / atoms)) if atoms else float("nan")
    print(f"{len(found)} structures, {sum(int((res.n_built > 0).sum()) for res in built)} side chains built ({suffix}), {atoms} atoms matched, "
          f"side-chain RMSD {total:.3f} Angstrom, {sum(res.pairs for res in built)} clashing pairs, {sum(unmatched)} unmatched rows "
          f"in {stats.get('submissions', 0)} GPU submission(s) -> {out}")
    return built


# (flag, argparse keywords)
CLI_FLAGS = (
    ("--path_to_pdb", dict(type=str, nargs="+", default=None, required=True,
                           help="PDB files and / or directories searched for *.pdb, *.pdb1, *.ent, each optionally .gz")),
    ("--path_to_output", dict(type=str, default="sidechains", help="directory for the built structures and the two csv files")),
    ("--path_to_pred_matrix", dict(type=str, default=None, help="338-column probability matrix written by predict.py --predict_rotamers (<model>_rot.csv)")),
    ("--path_to_datasetmap", dict(type=str, default="datasetmap.txt", help="the dataset map of the matrix (.txt): csv rows pdb, chain, residue number, label")),
    ("--chi", dict(type=str, default="class_centres", choices=("native", "class_centres"),
                   help="without a matrix: rebuild the native classes at their bin centres, or the native angles")),
    ("--clash_distance", dict(type=float, default=sidechains.CLASH_DISTANCE, help="two atoms closer than this (Angstrom) clash")),
    ("--device", dict(type=int, default=0, help="HIP device index")),
    ("--workers", dict(type=int, default=8, help="host threads that read and parse the files (at most 16)")),
    ("--lddt", dict(default=argparse.SUPPRESS, action="store_true",
                    help="also write structure_sidechain_lddt.csv and residue_sidechain_lddt.csv: the all-atom lDDT of every built structure "
                         "against its native, symmetric side-chain names resolved.  PARITY UNPINNED AGAINST OPENSTRUCTURE")),
)


def build_parser():
    parser = argparse.ArgumentParser(description="Side chains from rotamer classes, RMSD to the native and clashes, batched on the GPU (MI355X)",
                                     epilog=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for flag, keywords in CLI_FLAGS:
        parser.add_argument(flag, **keywords)
    return parser


if __name__ == "__main__":
    main(build_parser().parse_args())
