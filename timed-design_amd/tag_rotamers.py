"""tag_rotamers.py — rotamer labels of a set of PDB files: the chi angles of every residue and its class among the 338 rotamer
categories (design_utils.utils.get_rotamer_codec), computed on the GPU for all structures in as few th_tag_rotamers submissions
as the byte budget allows.  This is the labelling step of the reference's analyse_rotamers.py (design_utils/analyse_utils.py
tag_pdb_with_rot / extract_rotamer_encoding, which ask ampal) as a program of its own.

    python tag_rotamers.py --path_to_pdb biounits/ extra/1ubq.pdb1.gz --path_to_output rotamers

Writes ``rotamer_labels.json`` — {"<first four characters of the file's stem><chain>": [class index or null, ...]}, the file
analyse_rotamers.py reads with --path_to_rotamer_labels — and ``chi_angles.csv`` (structure, chain, residue, name, chi1..chi4 in
degrees, rotamer, class; empty fields stand for absent angles and unlabelled residues).

The rule — atom paths, bin edges (bin 1: 0 <= chi < 120, bin 3: -120 <= chi < 0, bin 2: the rest), the ALA / GLY class — is this
project's reading of ampal 1.5, written out in timed_hip/structure.py: PARITY UNPINNED AGAINST AMPAL, which is not available to
pin it.  ALA and GLY carry their single class ALA_0 / GLY_0; --no_ala_gly_class leaves them unlabelled.
"""
import argparse
import csv
import json
import sys
from pathlib import Path

from timed_hip import batching, structure
from timed_hip.pdbio import find_structures, stem_of


def main(args):
    found = find_structures(args.path_to_pdb)
    if not found:
        sys.exit(f"no *.pdb / *.pdb1 / *.ent (.gz) file under {args.path_to_pdb}")
    layouts = batching.parse_each(lambda item: structure.rotamer_layout(structure.first_model(item[1])), found, args.workers)
    stats = {}
    tagged = structure.tag_rotamers(layouts, device=args.device, ala_gly_class=not args.no_ala_gly_class, stats=stats)
    out = Path(args.path_to_output)
    out.mkdir(parents=True, exist_ok=True)
    labels = {}
    with open(out / "chi_angles.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["structure", "chain", "residue", "name", "chi1", "chi2", "chi3", "chi4", "rotamer", "class"])
        for (label, _), res in zip(found, tagged):
            mine = {}
            for r, c, chi, rot in zip(res.residues, res.cls.tolist(), res.chi, res.rotamers):
                w.writerow([label, r.chain, r.number, r.name] + ["" if x != x else repr(float(x)) for x in chi] +
                           ["" if rot is None else rot, "" if c < 0 else c])
                mine.setdefault(stem_of(label)[:4] + r.chain, []).append(None if c < 0 else int(c))
            labels.update(mine)                      # a later file with the same key replaces the earlier one, as the reference's dict does
    with open(out / "rotamer_labels.json", "w") as f:
        json.dump(labels, f)
        f.write("\n")
    n_res = sum(len(res.residues) for res in tagged)
    print(f"{len(found)} structures, {n_res} residues, {sum(int((res.cls >= 0).sum()) for res in tagged)} labelled "
          f"in {stats.get('submissions', 0)} GPU submission(s) -> {out}")
    return tagged


# (flag, argparse keywords)
CLI_FLAGS = (
    ("--path_to_pdb", dict(type=str, nargs="+", default=None, required=True,
                           help="PDB files and / or directories searched for *.pdb, *.pdb1, *.ent, each optionally .gz")),
    ("--path_to_output", dict(type=str, default="rotamers", help="directory for rotamer_labels.json and chi_angles.csv")),
    ("--device", dict(type=int, default=0, help="HIP device index")),
    ("--workers", dict(type=int, default=8, help="host threads that read and parse the files (at most 16)")),
    ("--no_ala_gly_class", dict(default=False, action="store_true", help="leave ALA and GLY unlabelled instead of ALA_0 / GLY_0")),
)


def build_parser():
    parser = argparse.ArgumentParser(description="Chi angles and rotamer classes of PDB structures, batched on the GPU (MI355X)",
                                     epilog=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for flag, keywords in CLI_FLAGS:
        parser.add_argument(flag, **keywords)
    return parser


if __name__ == "__main__":
    main(build_parser().parse_args())
