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

--secondary_structure additionally writes ``residue_secondary_structure.csv`` — structure, chain, residue number, residue name, the
class letter (H alpha-helix, G 3-10 helix, I pi-helix, E strand, B isolated bridge, T turn, S bend, - none), the three-state letter (H
helix: H G I; E strand: E B; C coil: the rest), the two lowest bridge partners as chain:number, the hydrogen bonds the residue accepts
(C=O) and donates (N-H) — and ``structure_secondary_structure.csv`` — structure, residues, n_hbonds, the number of residues of each
of the eight classes and the helix / strand / coil fractions; with --path_to_pred_matrix + --path_to_datasetmap also the mean
prediction entropy over the helix, the strand and the coil residues (NaN where a state is empty or no row pairs).  Rows pair with
residues by chain and residue number: with --support_old_datasetmap every map row names them, and the rows used are those whose pdb
code, or pdb code + chain, equals the file's stem; the two-column map names neither, so the rows of the key that equals the stem pair
by position, and only when there are as many as residues.  The residues are the non-hetero residues of EVERY chain (bridges pair
chains), whatever --all_chains says about the packing density.  The other two files keep their bytes.

PARITY UNPINNED AGAINST DSSP (mkdssp, PyMOL's dss, STRIDE): none of them is available to pin this against.  The rule is this project's
reading of the published definition (Kabsch & Sander 1983), written out in include/timed_hip.h and timed_hip/secstruct.py: every
hydrogen bond below -0.5 kcal/mol counts (no cap per residue), beta-bulges are not bridged over, priority H > E > B > G > I > T > S.
Assignments can differ from those programs' at helix ends and sheet edges.

--sasa additionally writes ``residue_sasa.csv`` — structure, chain, residue number, residue name, the solvent-accessible area of the
residue in square Angstrom, its polar (N and O atoms), apolar and backbone (N, CA, C, O) parts, the relative accessibility rsa (area /
the residue's maximum after Tien et al. 2013, a table WRITTEN FROM MEMORY, NOT FETCHED; not clamped; NaN for a residue outside it), the
burial letter (C core: rsa < --rsa_core; S surface: rsa >= --rsa_surface; B boundary; ? unknown — a convention, not a measurement) and
with --sasa_interface the area the residue loses in the complex — and ``structure_sasa.csv`` — structure, atoms, residues, the total,
polar and apolar area, the apolar share, the number of core, boundary and surface residues, the atoms without an exposed point, with
--sasa_interface the buried interface area (the chains alone minus the complex) and with --path_to_pred_matrix + --path_to_datasetmap
the mean prediction entropy over the core, boundary and surface residues, rows paired with residues as for --secondary_structure.
Shrake & Rupley (1973) with --sasa_points golden-spiral points per atom and a probe of --sasa_probe: th_sasa, every structure in one
batch.  The atoms are the non-hydrogen atoms of the non-hetero residues of EVERY chain; --sasa_hetero lets the non-water hetero atoms
occlude too.  The other files keep their bytes.

PARITY UNPINNED AGAINST FREESASA / NACCESS / DSSP / BIOPYTHON: none of them is available to pin this against.  The rule is this
project's own, written out in include/timed_hip.h and timed_hip/sasa.py: element radii after Bondi, strict inequalities, a point exactly
on a neighbour's sphere is exposed.  Areas differ from those programs' in detail.

Out of scope here: the reference script's CE-align RMSD (PyMOL), which is analyse_models.py --cealign, and its parsing of AlphaFold2
file names into model / temperature / sample / rank columns — the ``structure`` column is the file's path relative to the
--path_to_pdb entry it was found under.
"""
import argparse
import csv
import sys
from pathlib import Path

import numpy as np

from timed_hip import batching, sasa, secstruct, structure
from timed_hip.pdbio import PDB_SUFFIXES, find_structures, is_pdb_name, stem_of  # noqa: F401  (their home; kept importable from here)
from timed_hip.textio import float_repr as _fmt


SECSTRUCT_RESIDUE_COLUMNS = ["structure", "chain", "residue_number", "residue_name", "class", "three_state", "bridge_partner_1", "bridge_partner_2",
                             "bonds_accepted", "bonds_donated"]
SECSTRUCT_COLUMNS = ["structure", "residues", "n_hbonds", "n_none", "n_H", "n_B", "n_E", "n_G", "n_I", "n_T", "n_S", "helix_fraction",
                     "strand_fraction", "coil_fraction"]
SECSTRUCT_ENTROPY_COLUMNS = ["entropy_helix_mean", "entropy_strand_mean", "entropy_coil_mean"]
SASA_RESIDUE_COLUMNS = ["structure", "chain", "residue_number", "residue_name", "area", "polar_area", "apolar_area", "backbone_area", "rsa", "burial"]
SASA_COLUMNS = ["structure", "atoms", "residues", "total_area", "polar_area", "apolar_area", "apolar_share", "n_core", "n_boundary", "n_surface",
                "buried_atoms"]
SASA_ENTROPY_COLUMNS = ["entropy_core_mean", "entropy_boundary_mean", "entropy_surface_mean"]


def paired_entropy(label, residues, entropy, map_rows):
    """{index into ``residues``: the prediction entropy of the row that pairs with it}.  ``entropy``: {map key: entropy of each of its
    rows}; ``map_rows``: {map key: its (pdb, chain, number, label) rows} of an old-format map, or None for a two-column map.  See the
    module docstring for how rows pair with residues."""
    stem = stem_of(label)
    values = {}
    if map_rows is not None:
        index = {}
        for k, r in enumerate(residues):
            index.setdefault((r.chain, r.number), k)
        for key, rows in map_rows.items():
            if key != stem and str(rows[0][0]) != stem:
                continue
            for row, v in zip(rows, entropy[key]):
                k = index.get((str(row[1]).strip(), str(row[2]).strip()))
                if k is not None:
                    values.setdefault(k, float(v))
    else:
        e = entropy.get(stem)
        if e is not None and len(e) == len(residues):
            values = {k: float(v) for k, v in enumerate(e)}
    return values


def class_entropy(values, classes, order):
    """the mean of ``values`` (``paired_entropy``) over the residues of each class of ``order``; NaN where a class has no paired row"""
    out = []
    for state in order:
        mine = [values[k] for k, s in enumerate(classes) if s == state and k in values]
        out.append(float(np.mean(mine)) if mine else float("nan"))
    return out


def state_entropy(label, res, entropy, map_rows):
    """The mean prediction entropy over the helix, strand and coil residues of one assigned structure (NaN for an empty state)."""
    return class_entropy(paired_entropy(label, res.residues, entropy, map_rows), secstruct.three_state(res.cls).tolist(), (1, 2, 0))


def write_sasa(out, found, measured, interface=False, entropy=None, map_rows=None):
    """residue_sasa.csv and structure_sasa.csv"""
    with open(out / "residue_sasa.csv", "w", newline="") as fr, open(out / "structure_sasa.csv", "w", newline="") as fs:
        wr, ws = csv.writer(fr), csv.writer(fs)
        wr.writerow(SASA_RESIDUE_COLUMNS + (["area_lost_in_complex"] if interface else []))
        ws.writerow(SASA_COLUMNS + (["interface_area"] if interface else []) + (SASA_ENTROPY_COLUMNS if entropy is not None else []))
        for (label, _), res in zip(found, measured):
            letters = res.burial_letters
            for k, r in enumerate(res.residues):
                row = [label, r.chain, r.number, r.name] + [_fmt(v[k]) for v in (res.residue_area, res.polar_area, res.apolar_area, res.backbone_area,
                                                                                 res.rsa)] + [letters[k]]
                wr.writerow(row + ([_fmt(res.area_lost[k])] if interface else []))
            row = [label, len(res.exposed), len(res.residues), _fmt(res.total_area), _fmt(res.total_polar_area), _fmt(res.total_apolar_area),
                   _fmt(res.apolar_share)] + list(res.counts) + [res.n_buried_atoms]
            if interface:
                row.append(_fmt(res.interface_area))
            if entropy is not None:
                row += [_fmt(v) for v in class_entropy(paired_entropy(label, res.residues, entropy, map_rows), res.burial.tolist(), (0, 1, 2))]
            ws.writerow(row)


def write_secondary_structure(out, found, assigned, entropy=None, map_rows=None):
    """residue_secondary_structure.csv and structure_secondary_structure.csv"""
    with open(out / "residue_secondary_structure.csv", "w", newline="") as fr, open(out / "structure_secondary_structure.csv", "w", newline="") as fs:
        wr, ws = csv.writer(fr), csv.writer(fs)
        wr.writerow(SECSTRUCT_RESIDUE_COLUMNS)
        ws.writerow(SECSTRUCT_COLUMNS + (SECSTRUCT_ENTROPY_COLUMNS if entropy is not None else []))
        for (label, _), res in zip(found, assigned):
            names = [f"{r.chain}:{r.number}" for r in res.residues]
            letters, three = secstruct.as_string(res.cls), secstruct.as_string(res.cls, three=True)
            for k, r in enumerate(res.residues):
                first, second = (names[j] if j >= 0 else "" for j in res.partners[k].tolist())
                wr.writerow([label, r.chain, r.number, r.name, letters[k], three[k], first, second, int(res.accepted[k]), int(res.donated[k])])
            row = [label, len(res.residues), res.n_hbonds] + [int(c) for c in res.counts] + [_fmt(f) for f in res.fractions]
            if entropy is not None:
                row += [_fmt(v) for v in state_entropy(label, res, entropy, map_rows)]
            ws.writerow(row)


def main(args):
    with_secstruct = getattr(args, "secondary_structure", False)
    with_sasa = getattr(args, "sasa", False)
    if with_sasa and not 1 <= getattr(args, "sasa_points", 96) <= sasa.MAX_POINTS:
        sys.exit(f"--sasa_points {args.sasa_points} is outside 1 .. {sasa.MAX_POINTS}")
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
        return (model, structure.layout(model, args.atom_filter_function, include_hetero=True, all_chains=args.all_chains),
                secstruct.backbone_layout(model) if with_secstruct else None,
                sasa.atom_layout(model, include_hetero=getattr(args, "sasa_hetero", False)) if with_sasa else None)
    parsed = batching.parse_each(parse, found, args.workers)
    stats = {}
    budget = int(args.batch_mb * (1 << 20))
    results = structure.packing_density_layouts([p[1] for p in parsed], radius=args.radius, device=args.device, budget_bytes=budget, stats=stats)
    out = Path(args.path_to_output)
    out.mkdir(parents=True, exist_ok=True)
    map_rows = None
    if entropy is not None and args.support_old_datasetmap and (with_secstruct or with_sasa):
        from design_utils.utils import load_datasetmap
        map_rows = {}
        for row in load_datasetmap(Path(args.path_to_datasetmap), is_old=True):
            map_rows.setdefault(str(row[0]) + str(row[1]), []).append(row)
    if with_secstruct:
        assigned = secstruct.secondary_structure_layouts([p[2] for p in parsed], device=args.device, budget_bytes=budget, stats=stats)
        write_secondary_structure(out, found, assigned, entropy, map_rows)
    if with_sasa:
        interface = getattr(args, "sasa_interface", False)
        measured = sasa.sasa_layouts([p[3] for p in parsed], probe=getattr(args, "sasa_probe", 1.4), n_points=getattr(args, "sasa_points", 96),
                                     device=args.device, core=getattr(args, "rsa_core", 0.2), surface=getattr(args, "rsa_surface", 0.5),
                                     interface=interface, budget_bytes=budget, stats=stats)
        write_sasa(out, found, measured, interface, entropy, map_rows)
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
    # absent from the namespace unless given: a namespace built by an older caller has no such attribute either
    ("--secondary_structure", dict(default=argparse.SUPPRESS, action="store_true",
                                   help="also write residue_secondary_structure.csv and structure_secondary_structure.csv: the DSSP class "
                                        "(H G I E B T S -) and three-state letter of every residue of every chain, its bridge partners and "
                                        "hydrogen bonds, and per structure the counts and the helix / strand / coil fractions (with a prediction "
                                        "matrix: the mean entropy of each state).  PARITY UNPINNED AGAINST DSSP")),
    ("--sasa", dict(default=argparse.SUPPRESS, action="store_true",
                    help="also write residue_sasa.csv and structure_sasa.csv: the solvent-accessible surface area (Shrake & Rupley) of every "
                         "residue of every chain, its polar, apolar and backbone parts, its relative accessibility and burial class "
                         "(C core, B boundary, S surface), and per structure the areas, the apolar share and the class counts (with a "
                         "prediction matrix: the mean entropy of each class).  PARITY UNPINNED AGAINST FREESASA / NACCESS / DSSP / BIOPYTHON")),
    ("--sasa_points", dict(default=argparse.SUPPRESS, type=int, help="--sasa: golden-spiral points per atom, 1 .. 1024 (default 96)")),
    ("--sasa_probe", dict(default=argparse.SUPPRESS, type=float, help="--sasa: probe radius in Angstrom (default 1.4; 0: the van der Waals surface)")),
    ("--sasa_hetero", dict(default=argparse.SUPPRESS, action="store_true", help="--sasa: non-water hetero atoms occlude too (waters never do)")),
    ("--sasa_interface", dict(default=argparse.SUPPRESS, action="store_true",
                              help="--sasa: also measure every chain of a complex alone: the area each residue loses in the complex and the "
                                   "buried interface area of the structure")),
    ("--rsa_core", dict(default=argparse.SUPPRESS, type=float, help="--sasa: a residue is core below this relative accessibility (default 0.2)")),
    ("--rsa_surface", dict(default=argparse.SUPPRESS, type=float, help="--sasa: a residue is surface from this relative accessibility (default 0.5)")),
)


def build_parser():
    parser = argparse.ArgumentParser(description="Packing density and B-factor of PDB structures, batched on the GPU (MI355X)",
                                     epilog=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for flag, keywords in CLI_FLAGS:
        parser.add_argument(flag, **keywords)
    return parser


if __name__ == "__main__":
    main(build_parser().parse_args())
