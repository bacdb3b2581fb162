"""analyse_models.py — score structure models against their native backbone: RMSD after superposition, the GDT fractions and the
deviation of every residue, for all pairs in as few th_superpose submissions as the byte budget allows.  This is the step of the
reference's evaluation chain that scripts/analyse_af2.py does one PyMOL call at a time (calculate_RMSD_and_gdt: cmd.align on the CA
atoms, then the fractions of aligned pairs within 1, 2, 4 and 8 Angstrom).

    python analyse_models.py --path_to_reference native/1ubq.pdb1.gz --path_to_models af2_models/ --path_to_output scores
    python analyse_models.py --pairs pairs.csv --path_to_output scores

--pairs reads lines of ``reference_path,model_path[,label]`` (relative paths are taken from the CSV's directory).  Every file is
parsed once, on host threads, however many pairs name it.

Writes ``model_scores.csv``, one row per pair — label, reference, model, n_valid, n_kept, cycles_run, rmsd_kept (the number
cmd.align returns: over the positions the refinement kept), rmsd_all (every position under that final fit), rmsd_fit_all (the
conventional CA RMSD: one fit over every position), gdt_1, gdt_2, gdt_4, gdt_8 and mean_gdt (the reference's column),
sequence_identity (the reference's seq_accuracy), unpaired_reference, unpaired_model, error — and ``residue_deviation.csv`` — label,
chain, residue number (of the reference), the distance d_i under the final fit and whether the refinement kept the position.

PARITY UNPINNED AGAINST PYMOL: PyMOL is not available to pin this against.  The rule is this project's reading of the documented
behaviour of cmd.align (cycles 5, cutoff 2.0), written out in include/timed_hip.h and timed_hip/superpose.py: a least-squares fit
with a proper rotation, then up to --cycles rounds that drop positions further than --cutoff x RMS and fit again.  Pairing is by
position (file order; native and model must be equally long, as the reference asserts) or by number (chain, residue number and
insertion code), NOT by a sequence alignment unless --pair_by_seqalign asks for one (below).  Out of scope: AlphaFold2 folder layouts and parsing FASTA or file names into model /
temperature / sample columns — the label is the model's path below --path_to_models, or the third CSV field.

--lddt additionally writes ``model_lddt.csv``, one row per pair — label, reference, model, n_valid, n_included (ordered pairs of
positions closer than --lddt_radius in the reference), lddt, the fractions of those pairs preserved within 0.5, 1, 2 and 4 Angstrom,
mean_model_bfactor (over the paired positions that have one), error — and ``residue_lddt.csv`` — label, chain, number and residue name
(of the reference), n_included, lddt and model_bfactor of every position.  The score is superposition-free: it compares distances
within each structure and never fits one on the other, so a re-oriented domain costs only the pairs across its hinge — and a mirror
image, which the fit above rejects with a large RMSD, scores 1.0.  That is the reason to report both.  model_bfactor is the model's
B-factor of the paired atom as stored; AlphaFold2 writes its own PREDICTION of this score there (pLDDT, 0-100), lddt is the
measured one (0-1).  Both scores come from one parse of every file that can be read.

PARITY UNPINNED AGAINST OPENSTRUCTURE: neither OpenStructure nor AlphaFold's lddt.py is available to pin this against.  The rule is
this project's reading of the published definition (Mariani et al. 2013) in the CA-only form AlphaFold uses, written out in
include/timed_hip.h and timed_hip/lddt.py: one position per residue, no stereochemistry checks, strict inequalities on both tests, the
global score weighted by pairs (not the mean of the per-residue scores).

--tmscore additionally writes ``model_tmscore.csv``, one row per pair — label, reference, model, n_valid, norm_length (the residues
of the reference that have a CA atom: what the model lacks of them costs score), d0, tm_score, tm_global_fit (the same sum under the
ONE least-squares fit over all positions, th_superpose with cycles 0: beside tm_score it shows what the search bought), n_seeds, n_fits,
error.  TM-score is the maximum over superpositions of sum 1 / (1 + (d_i / d0)^2) / norm_length; the superposition that attains it is
searched for from every window of the chain (--tm_rounds refinement rounds per seed at most), a re-oriented domain costs only its own
positions, and a mirror image scores low (the rotation is proper).  At most 4096 positions per pair.  The files parsed for the
superposition are reused.

PARITY UNPINNED AGAINST THE TM-score PROGRAM: Zhang & Skolnick's TMscore is not available to pin this against.  The rule is this
project's reading of the published definition and search, written out in include/timed_hip.h and timed_hip/tmscore.py.  It aligns no
sequences (that is TM-align).

--cealign additionally writes ``model_cealign.csv``, one row per pair — label, reference, model, n_ref, n_model (the positions of either
structure), n_starts (fragment pairs similar enough to start a path), n_afps, n_aligned (8 per aligned fragment pair), rmsd (over the
aligned positions: the number cmd.cealign returns), path_score, error — and ``residue_cealign.csv`` — label, chain, number and residue
of every residue of the reference, the chain, number and residue of the model's residue aligned to it (empty if none) and their
distance under the winning fit.  This is the reference's calculate_RMSD_and_gdt / _calculate_RMSD of scripts/analyse_all_properties.py:
a sequence-independent structural alignment (CE, Shindyalov & Bourne 1998) of the CA atoms, for which the two chains need be neither
equally long nor numbered alike (at most 2048 positions each).  --ce_d0, --ce_d1 and --ce_gap_max are its thresholds.
--pair_by_cealign makes that alignment the pairing of model_scores.csv, of --lddt and of --tmscore, in place of --pair_by: a length
mismatch is then no error, and what either side has outside the alignment counts as unpaired.

PARITY UNPINNED AGAINST PYMOL: the rule of --cealign is this project's reading of the published CE algorithm with cealign's documented
defaults (window 8, d0 3.0, d1 4.0, gap_max 30, the best 20 paths re-scored by RMSD), written out in include/timed_hip.h and
timed_hip/cealign.py.

--secondary_structure additionally writes ``model_secstruct.csv``, one row per pair — label, reference, model, n_paired, q8 and q3 (the
share of the paired positions whose DSSP class, and whose three-state reduction helix / strand / coil, agree), the helix and strand
fractions and the number of backbone hydrogen bonds of either structure (over ALL of its residues that have a CA atom, paired or
not), error — and ``residue_secstruct.csv`` — label, chain, number and residue of the reference's residue of every paired position, its
class and the model's, both three-state letters, and the chain and number of the model's residue.  Did the model keep the native's
helices and strands?  Each distinct file is assigned once, from the structures already parsed for the superposition, so a native
shared by a thousand models is one structure in the batch; the pairing is that of model_scores.csv (--pair_by, or --pair_by_cealign).

--seqalign additionally writes ``model_seqalign.csv``, one row per pair — label, reference, model, n_ref, n_model (the residues of
either structure that have a CA atom), score (in units of the table: twice BLOSUM62's), n_aligned, identity (n_identical / n_aligned),
positives (aligned with a positive table entry, over n_aligned), n_gaps and n_gap_residues (runs of unpaired residues of either side
between the first and the last aligned pair, and the residues in them), coverage_ref and coverage_model (n_aligned over either length),
error — and ``residue_seqalign.csv`` — label, chain, number and residue of every residue of the reference, and the chain, number and
residue of the model's residue aligned to it (empty if none).  This is the alignment step of cmd.align: the SEQUENCES of the two
structures (chains concatenated in file order, residue names as one-letter codes, anything unknown as X) are aligned globally with
affine gap costs — 2 x BLOSUM62, a run of k unpaired residues costs 2 x (--sa_gap_open + (k - 1) --sa_gap_extend), cmd.align's
documented 10 and 0.5 — with free ends, or charged ends under --sa_global (th_seqalign, at most 4096 residues each).
--pair_by_seqalign makes that alignment the pairing of model_scores.csv and of every optional score, in place of --pair_by: it
survives renumbering, a missing loop and a purification tag together, and unlike --pair_by_cealign it exists for a misfolded model.
It cannot be combined with --pair_by_cealign.

PARITY UNPINNED AGAINST PYMOL: cmd.align's own recurrences, end-gap treatment and tie handling are not available to pin --seqalign
against; the rule is this project's own, written out in include/timed_hip.h and timed_hip/seqalign.py.  Out of scope: local, profile
and multiple alignment, banded or heuristic search.

PARITY UNPINNED AGAINST DSSP (mkdssp, PyMOL's dss, STRIDE): none of them is available to pin this against.  The rule is this project's
reading of the published definition (Kabsch & Sander 1983), written out in include/timed_hip.h and timed_hip/secstruct.py: every
hydrogen bond below -0.5 kcal/mol counts, beta-bulges are not bridged over, priority H > E > B > G > I > T > S.

--sasa additionally writes ``model_sasa.csv``, one row per pair — label, reference, model, n_paired, the total and the apolar
solvent-accessible area of either structure (over ALL of its residues that have a CA atom, paired or not), burial_agreement (the share of
the paired positions in the same burial class: core, boundary, surface), mean_abs_rsa_difference and rsa_correlation (Pearson; NaN under
2 positions) of the relative accessibilities of the paired positions, error — and ``residue_sasa.csv`` — label, chain, number and residue
of the reference's residue of every paired position, the area, the relative accessibility and the burial letter (C, B, S, ?) of both
sides, and the chain and number of the model's residue.  Did the model bury what the native buries?  Shrake & Rupley (1973) with
--sasa_points golden-spiral points per atom and a probe of --sasa_probe (th_sasa); the atoms are the non-hydrogen atoms of the residues
already parsed for the superposition (hetero atoms never occlude here, and chains are not measured alone: analyse_properties.py has
--sasa_hetero and --sasa_interface).  Each distinct file goes through the kernel once; the pairing is that of model_scores.csv.

PARITY UNPINNED AGAINST FREESASA / NACCESS / DSSP / BIOPYTHON: none of them is available to pin this against.  The rule is this
project's own, written out in include/timed_hip.h and timed_hip/sasa.py; the maximum areas behind the relative accessibility (after
Tien et al. 2013) are WRITTEN FROM MEMORY, NOT FETCHED.

--lddt_all_atom additionally writes ``model_lddt_all_atom.csv``, one row per pair — label, reference, model, n_atoms (the reference's
heavy atoms of the paired residues with finite coordinates), n_missing (of those, atoms the model lacks: they cost score),
n_mismatched_residues (paired residues whose names differ: only their N, CA, C, O enter), n_included, lddt, the four preserved
fractions, lddt_backbone and lddt_sidechain (the same sums over the rows of N, CA, C, O and of the other atoms), n_swapped_residues,
error — and ``residue_lddt_all_atom.csv`` — label, chain, number and residue of the reference, the model's residue, n_atoms, n_missing,
n_included, lddt and swapped of every paired residue.  This is the lDDT that CASP, CAMEO and OpenStructure quote (th_lddt_atoms):
over all heavy atoms, pairs inside one residue excluded, with the names of symmetric side-chain atoms (ASP OD1/OD2, GLU OE1/OE2, PHE
and TYR CD1/CD2 and CE1/CE2, ARG NH1/NH2, LEU CD1/CD2, VAL CG1/CG2) resolved per residue, so a ring turned by 180 degrees is not
charged; --lddt_no_symmetry scores the model as named.  It reuses --lddt_radius, --pair_by and --pair_by_cealign and the files parsed
for the superposition.  PARITY UNPINNED AGAINST OPENSTRUCTURE: the rule is this project's reading of the published definition,
written out in include/timed_hip.h and timed_hip/lddt_atoms.py; the table of symmetric atoms is WRITTEN FROM MEMORY, NOT FETCHED.  Out
of scope: stereochemistry checks, sequence-separation filters, ligands, sequence alignment, hydrogens, NMR ensembles.
"""
import argparse
import csv
import sys
from pathlib import Path

import numpy as np

from timed_hip import cealign as cealign_module
from timed_hip import lddt as lddt_module
from timed_hip import lddt_atoms as lddt_atoms_module
from timed_hip import sasa as sasa_module
from timed_hip import secstruct as secstruct_module
from timed_hip import seqalign as seqalign_module
from timed_hip import superpose
from timed_hip import tmscore as tmscore_module
from timed_hip.pdbio import find_structures
from timed_hip.textio import float_repr as _fmt

SCORE_COLUMNS = ["label", "reference", "model", "n_valid", "n_kept", "cycles_run", "rmsd_kept", "rmsd_all", "rmsd_fit_all", "gdt_1", "gdt_2",
                 "gdt_4", "gdt_8", "mean_gdt", "sequence_identity", "unpaired_reference", "unpaired_model", "error"]
RESIDUE_COLUMNS = ["label", "chain", "residue_number", "distance", "kept"]
LDDT_COLUMNS = ["label", "reference", "model", "n_valid", "n_included", "lddt", "preserved_0.5", "preserved_1", "preserved_2", "preserved_4",
                "mean_model_bfactor", "error"]
RESIDUE_LDDT_COLUMNS = ["label", "chain", "number", "residue", "n_included", "lddt", "model_bfactor"]
CEALIGN_COLUMNS = ["label", "reference", "model", "n_ref", "n_model", "n_starts", "n_afps", "n_aligned", "rmsd", "path_score", "error"]
RESIDUE_CEALIGN_COLUMNS = ["label", "chain", "number", "residue", "model_chain", "model_number", "model_residue", "distance"]
SEQALIGN_COLUMNS = ["label", "reference", "model", "n_ref", "n_model", "score", "n_aligned", "identity", "positives", "n_gaps", "n_gap_residues",
                    "coverage_ref", "coverage_model", "error"]
RESIDUE_SEQALIGN_COLUMNS = ["label", "chain", "number", "residue", "model_chain", "model_number", "model_residue"]
TMSCORE_COLUMNS = ["label", "reference", "model", "n_valid", "norm_length", "d0", "tm_score", "tm_global_fit", "n_seeds", "n_fits", "error"]
SECSTRUCT_COLUMNS = ["label", "reference", "model", "n_paired", "q8", "q3", "reference_helix_fraction", "reference_strand_fraction",
                     "model_helix_fraction", "model_strand_fraction", "reference_n_hbonds", "model_n_hbonds", "error"]
RESIDUE_SECSTRUCT_COLUMNS = ["label", "chain", "number", "residue", "reference_class", "model_class", "reference_three_state", "model_three_state",
                             "model_chain", "model_number"]
SASA_COLUMNS = ["label", "reference", "model", "n_paired", "reference_total_area", "reference_apolar_area", "model_total_area", "model_apolar_area",
                "burial_agreement", "mean_abs_rsa_difference", "rsa_correlation", "error"]
RESIDUE_SASA_COLUMNS = ["label", "chain", "number", "residue", "reference_area", "model_area", "reference_rsa", "model_rsa", "reference_burial",
                        "model_burial", "model_chain", "model_number"]


def read_pairs(path):
    """[(label, reference path, model path)] of a --pairs CSV; empty lines and lines starting with # are skipped"""
    path = Path(path)
    out = []
    with open(path, newline="") as f:
        for row in csv.reader(f):
            row = [field.strip() for field in row]
            if not row or not any(row) or row[0].startswith("#"):
                continue
            if len(row) < 2 or not row[0] or not row[1]:
                sys.exit(f"{path}: a line needs reference_path,model_path[,label], got {row}")
            ref, model = (p if p.is_absolute() else path.parent / p for p in (Path(row[0]), Path(row[1])))
            out.append((row[2] if len(row) > 2 and row[2] else row[1], ref, model))
    return out


def write_lddt(out, todo, scores):
    """model_lddt.csv and residue_lddt.csv"""
    with open(out / "model_lddt.csv", "w", newline="") as fs, open(out / "residue_lddt.csv", "w", newline="") as fr:
        ws, wr = csv.writer(fs), csv.writer(fr)
        ws.writerow(LDDT_COLUMNS)
        wr.writerow(RESIDUE_LDDT_COLUMNS)
        for (label, ref, model), res in zip(todo, scores):
            known = res.model_bfactor[res.model_bfactor == res.model_bfactor]
            ws.writerow([label, str(ref), str(model), res.n_valid, res.n_included, _fmt(res.lddt)] + [_fmt(p) for p in res.preserved]
                        + [_fmt(known.mean() if len(known) else float("nan")), res.error or ""])
            for r, n, score, b in zip(res.residues, res.n_i.tolist(), res.lddt_i, res.model_bfactor):
                wr.writerow([label, r.chain, r.number, r.name, n, _fmt(score), _fmt(b)])


def write_secstruct(out, todo, prepared, device, stats):
    """model_secstruct.csv and residue_secstruct.csv: every distinct structure of ``prepared`` is assigned once, in one batch"""
    distinct = {}
    for item in prepared.pairs:
        if not isinstance(item, str):
            for side in item[:2]:
                distinct.setdefault(id(side), side)
    assigned = secstruct_module.secondary_structure_layouts([secstruct_module.layout_of_residues(side.residues) for side in distinct.values()],
                                                            device=device, stats=stats)
    assigned = dict(zip(distinct, assigned))
    nan = float("nan")
    with open(out / "model_secstruct.csv", "w", newline="") as fs, open(out / "residue_secstruct.csv", "w", newline="") as fr:
        ws, wr = csv.writer(fs), csv.writer(fr)
        ws.writerow(SECSTRUCT_COLUMNS)
        wr.writerow(RESIDUE_SECSTRUCT_COLUMNS)
        for (label, ref, model), item in zip(todo, prepared.pairs):
            if isinstance(item, str):
                ws.writerow([label, str(ref), str(model), 0] + [_fmt(nan)] * 6 + [0, 0, item])
                continue
            ours, theirs = np.asarray(item[2], dtype=np.int64), np.asarray(item[3], dtype=np.int64)
            a, b = assigned[id(item[0])], assigned[id(item[1])]
            mine, other = a.cls[ours], b.cls[theirs]
            n = len(ours)
            q8 = float((mine == other).sum()) / n if n else nan
            q3 = float((secstruct_module.three_state(mine) == secstruct_module.three_state(other)).sum()) / n if n else nan
            ws.writerow([label, str(ref), str(model), n, _fmt(q8), _fmt(q3)] + [_fmt(f) for f in a.fractions[:2] + b.fractions[:2]]
                        + [a.n_hbonds, b.n_hbonds, ""])
            letters, three = (secstruct_module.as_string(mine), secstruct_module.as_string(other)), (
                secstruct_module.as_string(mine, three=True), secstruct_module.as_string(other, three=True))
            for k, (i, j) in enumerate(zip(ours.tolist(), theirs.tolist())):
                r, m = a.residues[i], b.residues[j]
                wr.writerow([label, r.chain, r.number, r.name, letters[0][k], letters[1][k], three[0][k], three[1][k], m.chain, m.number])


def pearson(a, b):
    """the Pearson correlation of two equally long sequences of numbers; NaN under 2 numbers or where either does not vary"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if len(a) < 2:
        return float("nan")
    da, db = a - a.mean(), b - b.mean()
    norm = float(np.sqrt((da * da).sum() * (db * db).sum()))
    return float((da * db).sum()) / norm if norm > 0 else float("nan")


def write_sasa(out, todo, prepared, args, stats):
    """model_sasa.csv and residue_sasa.csv: every distinct structure of ``prepared`` goes through the kernel once, in one batch"""
    distinct = {}
    for item in prepared.pairs:
        if not isinstance(item, str):
            for side in item[:2]:
                distinct.setdefault(id(side), side)
    measured = sasa_module.sasa_layouts([sasa_module.layout_of_residues(side.residues) for side in distinct.values()],
                                        probe=getattr(args, "sasa_probe", 1.4), n_points=getattr(args, "sasa_points", 96), device=args.device,
                                        core=getattr(args, "rsa_core", 0.2), surface=getattr(args, "rsa_surface", 0.5), stats=stats)
    measured = dict(zip(distinct, measured))
    nan = float("nan")
    with open(out / "model_sasa.csv", "w", newline="") as fs, open(out / "residue_sasa.csv", "w", newline="") as fr:
        ws, wr = csv.writer(fs), csv.writer(fr)
        ws.writerow(SASA_COLUMNS)
        wr.writerow(RESIDUE_SASA_COLUMNS)
        for (label, ref, model), item in zip(todo, prepared.pairs):
            if isinstance(item, str):
                ws.writerow([label, str(ref), str(model), 0] + [_fmt(nan)] * 7 + [item])
                continue
            ours, theirs = np.asarray(item[2], dtype=np.int64), np.asarray(item[3], dtype=np.int64)
            a, b = measured[id(item[0])], measured[id(item[1])]
            n = len(ours)
            mine, other = a.rsa[ours], b.rsa[theirs]
            known = ~(np.isnan(mine) | np.isnan(other))
            agreement = float((a.burial[ours] == b.burial[theirs]).sum()) / n if n else nan
            difference = float(np.abs(mine[known] - other[known]).mean()) if known.any() else nan
            ws.writerow([label, str(ref), str(model), n, _fmt(a.total_area), _fmt(a.total_apolar_area), _fmt(b.total_area), _fmt(b.total_apolar_area),
                         _fmt(agreement), _fmt(difference), _fmt(pearson(mine[known], other[known])), ""])
            letters = a.burial_letters, b.burial_letters
            for i, j in zip(ours.tolist(), theirs.tolist()):
                r, m = a.residues[i], b.residues[j]
                wr.writerow([label, r.chain, r.number, r.name, _fmt(a.residue_area[i]), _fmt(b.residue_area[j]), _fmt(a.rsa[i]), _fmt(b.rsa[j]),
                             letters[0][i], letters[1][j], m.chain, m.number])


def tm_sum(dist, d0, norm_length):
    """sum over the numbers of ``dist``, in index order, of 1 / (1 + (d / d0)^2), divided by ``norm_length``: NaN when there is none"""
    total, seen = 0.0, False
    for d in dist.tolist():
        if d == d:
            q = d / d0
            total += 1.0 / (1.0 + q * q)
            seen = True
    return total / norm_length if seen else float("nan")


def write_tmscore(out, todo, scores, global_fits):
    """model_tmscore.csv; ``global_fits``: the results of th_superpose with cycles = 0 for the same pairs"""
    with open(out / "model_tmscore.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(TMSCORE_COLUMNS)
        for (label, ref, model), res, once in zip(todo, scores, global_fits):
            whole = float("nan") if res.error or once.error else tm_sum(once.dist, res.d0, res.norm_length)
            w.writerow([label, str(ref), str(model), res.n_valid, res.norm_length, _fmt(res.d0), _fmt(res.tm), _fmt(whole), res.n_seeds, res.n_fits,
                        res.error or ""])


def write_cealign(out, todo, aligned):
    """model_cealign.csv and residue_cealign.csv; ``aligned``: what cealign.cealign returned, with the transforms"""
    with open(out / "model_cealign.csv", "w", newline="") as fs, open(out / "residue_cealign.csv", "w", newline="") as fr:
        ws, wr = csv.writer(fs), csv.writer(fr)
        ws.writerow(CEALIGN_COLUMNS)
        wr.writerow(RESIDUE_CEALIGN_COLUMNS)
        for (label, ref, model), res in zip(todo, aligned):
            ws.writerow([label, str(ref), str(model), res.n_ref, res.n_model, res.n_starts, res.n_afps, res.n_aligned, _fmt(res.rmsd),
                         _fmt(res.path_score), res.error or ""])
            if res.error:
                continue
            partner = dict(zip(res.reference_index.tolist(), res.model_index.tolist()))
            moved = res.model.xyz[res.model_index] @ res.transform[:, :3].T + res.transform[:, 3]
            delta = moved - res.reference.xyz[res.reference_index]
            distance = dict(zip(res.reference_index.tolist(), np.sqrt((delta * delta).sum(axis=1)).tolist()))
            for k, r in enumerate(res.reference.residues):
                m = res.model.residues[partner[k]] if k in partner else None
                wr.writerow([label, r.chain, r.number, r.name] + ([m.chain, m.number, m.name, _fmt(distance[k])] if m else ["", "", "", ""]))


def write_seqalign(out, todo, aligned):
    """model_seqalign.csv and residue_seqalign.csv; ``aligned``: what seqalign.align returned"""
    with open(out / "model_seqalign.csv", "w", newline="") as fs, open(out / "residue_seqalign.csv", "w", newline="") as fr:
        ws, wr = csv.writer(fs), csv.writer(fr)
        ws.writerow(SEQALIGN_COLUMNS)
        wr.writerow(RESIDUE_SEQALIGN_COLUMNS)
        for (label, ref, model), res in zip(todo, aligned):
            ws.writerow([label, str(ref), str(model), res.n_ref, res.n_model, res.score, res.n_aligned, _fmt(res.identity), _fmt(res.positives),
                         res.n_gaps, res.n_gap_residues, _fmt(res.coverage_ref), _fmt(res.coverage_model), res.error or ""])
            if res.error:
                continue
            partner = dict(zip(res.reference_index.tolist(), res.model_index.tolist()))
            for k, r in enumerate(res.reference.residues):
                m = res.model.residues[partner[k]] if k in partner else None
                wr.writerow([label, r.chain, r.number, r.name] + ([m.chain, m.number, m.name] if m else ["", "", ""]))


def seqalign_costs(args):
    """(gap_open, gap_extend) of th_seqalign from --sa_gap_open and --sa_gap_extend: twice each, which must be integers"""
    costs = []
    for flag, default in (("sa_gap_open", 10.0), ("sa_gap_extend", 0.5)):
        value = 2.0 * float(getattr(args, flag, default))
        if not value == int(value) or not 0 <= value <= 32767:
            sys.exit(f"--{flag} {getattr(args, flag, default)}: twice the cost must be an integer from 0 to 32767")
        costs.append(int(value))
    if costs[0] < costs[1]:
        sys.exit(f"--sa_gap_open {costs[0] / 2} is below --sa_gap_extend {costs[1] / 2}")
    return tuple(costs)


def main(args):
    if args.pairs:
        if args.path_to_reference or args.path_to_models:
            sys.exit("--pairs replaces --path_to_reference / --path_to_models")
        todo = read_pairs(args.pairs)
    else:
        if not (args.path_to_reference and args.path_to_models):
            sys.exit("give --path_to_reference FILE --path_to_models DIR_OR_FILES, or --pairs CSV")
        reference = Path(args.path_to_reference)
        if not reference.is_file():
            sys.exit(f"no reference file at {reference}")
        todo = [(label, reference, path) for label, path in find_structures(args.path_to_models)]
    if not todo:
        sys.exit("no pair to score: no *.pdb / *.pdb1 / *.ent (.gz) file under --path_to_models, or an empty --pairs file")
    if (args.lddt or getattr(args, "lddt_all_atom", False)) and not (args.lddt_radius > 0 and args.lddt_radius < float("inf")):
        sys.exit(f"--lddt_radius {args.lddt_radius} is not a positive finite number")
    if getattr(args, "sasa", False) and not 1 <= getattr(args, "sasa_points", 96) <= sasa_module.MAX_POINTS:
        sys.exit(f"--sasa_points {args.sasa_points} is outside 1 .. {sasa_module.MAX_POINTS}")
    if args.tmscore and args.tm_rounds < 0:
        sys.exit(f"--tm_rounds {args.tm_rounds} is negative")
    by_sequence = getattr(args, "pair_by_seqalign", False)
    if by_sequence and args.pair_by_cealign:
        sys.exit("--pair_by_seqalign and --pair_by_cealign both replace --pair_by: give one of them")
    sequence_aligning = getattr(args, "seqalign", False) or by_sequence
    if sequence_aligning:
        sa_gap_open, sa_gap_extend = seqalign_costs(args)
    aligning = args.cealign or args.pair_by_cealign
    if aligning and not (0 < args.ce_d0 < float("inf") and 0 < args.ce_d1 < float("inf")):
        sys.exit(f"--ce_d0 {args.ce_d0} and --ce_d1 {args.ce_d1} must be positive finite numbers")
    if aligning and not 0 <= args.ce_gap_max <= 31:
        sys.exit(f"--ce_gap_max {args.ce_gap_max} is outside 0 .. 31")
    stats = {}
    pairs = [(ref, model) for _, ref, model in todo]
    aligned = None
    if aligning:
        aligned = cealign_module.cealign(pairs, "CA", args.ce_d0, args.ce_d1, args.ce_gap_max, args.device, True, args.workers, stats=stats)
        pairs = [(res.reference or ref, res.model or model) for (ref, model), res in zip(pairs, aligned)]        # parsed once for all scores
    sequence_aligned = None
    if sequence_aligning:
        sequence_aligned = seqalign_module.align(pairs, "CA", None, sa_gap_open, sa_gap_extend, not getattr(args, "sa_global", False), args.device,
                                                 args.workers, stats=stats)
        pairs = [(res.reference or ref, res.model or model) for (ref, model), res in zip(pairs, sequence_aligned)]
    if by_sequence:
        prepared = seqalign_module.prepare_aligned(pairs, results=sequence_aligned, stats=stats)
    elif args.pair_by_cealign:
        prepared = cealign_module.prepare_aligned(pairs, results=aligned, stats=stats)
    else:
        prepared = superpose.prepare(pairs, args.pair_by, "CA", args.workers)     # read and paired once for both scores
    results = superpose.superpose(prepared, cycles=args.cycles, cutoff=args.cutoff, device=args.device, stats=stats)
    out = Path(args.path_to_output)
    out.mkdir(parents=True, exist_ok=True)
    if args.cealign:
        write_cealign(out, todo, aligned)
    if getattr(args, "seqalign", False):
        write_seqalign(out, todo, sequence_aligned)
    if args.lddt:
        write_lddt(out, todo, lddt_module.lddt(prepared, radius=args.lddt_radius, device=args.device, stats=stats))
    if getattr(args, "lddt_all_atom", False):
        lddt_atoms_module.write_csv(out / "model_lddt_all_atom.csv", out / "residue_lddt_all_atom.csv", todo,
                                    lddt_atoms_module.lddt_atoms(prepared, symmetry=not getattr(args, "lddt_no_symmetry", False),
                                                                 radius=args.lddt_radius, device=args.device, stats=stats))
    if args.secondary_structure:
        write_secstruct(out, todo, prepared, args.device, stats)
    if getattr(args, "sasa", False):
        write_sasa(out, todo, prepared, args, stats)
    if args.tmscore:
        write_tmscore(out, todo, tmscore_module.tmscore(prepared, rounds=args.tm_rounds, device=args.device, stats=stats),
                      superpose.superpose(prepared, cycles=0, device=args.device, stats=stats))
    with open(out / "model_scores.csv", "w", newline="") as fs, open(out / "residue_deviation.csv", "w", newline="") as fr:
        ws, wr = csv.writer(fs), csv.writer(fr)
        ws.writerow(SCORE_COLUMNS)
        wr.writerow(RESIDUE_COLUMNS)
        for (label, ref, model), res in zip(todo, results):
            ws.writerow([label, str(ref), str(model), res.n_valid, res.n_kept, res.cycles_run, _fmt(res.rmsd_kept), _fmt(res.rmsd_all),
                         _fmt(res.rmsd_fit_all)] + [_fmt(g) for g in res.gdt] + [_fmt(res.mean_gdt), _fmt(res.sequence_identity),
                                                                                res.unpaired_reference, res.unpaired_model, res.error or ""])
            for r, d, k in zip(res.residues, res.dist, res.kept.tolist()):
                wr.writerow([label, r.chain, r.number, _fmt(d), k])
    failed = sum(1 for res in results if res.error)
    print(f"{len(todo)} pairs ({failed} with an error), {sum(len(res.dist) for res in results)} positions, {stats.get('files_parsed', 0)} files parsed "
          f"in {stats.get('submissions', 0)} GPU submission(s) -> {out}")
    return results


# (flag, argparse keywords)
CLI_FLAGS = (
    ("--path_to_reference", dict(type=str, default=None, help="the native structure every model is scored against")),
    ("--path_to_models", dict(type=str, nargs="+", default=None,
                              help="model files and / or directories searched recursively for *.pdb, *.pdb1, *.ent, each optionally .gz")),
    ("--pairs", dict(type=str, default=None, help="CSV of reference_path,model_path[,label] lines instead of the two options above")),
    ("--cycles", dict(type=int, default=5, help="outlier-rejection refinement cycles at most (default 5, cmd.align's; 0: one fit over all)")),
    ("--cutoff", dict(type=float, default=2.0, help="a refinement cycle drops positions further than this many RMS (default 2.0, cmd.align's)")),
    ("--pair_by", dict(type=str, default="position", choices=list(superpose.PAIR_BY),
                       help="position: CA atoms in file order, equal length required (default); number: by chain, residue number and "
                            "insertion code.  Neither is a sequence alignment: that is --pair_by_seqalign")),
    ("--device", dict(type=int, default=0, help="HIP device index")),
    ("--workers", dict(type=int, default=8, help="host threads that read and parse the files (at most 16)")),
    ("--path_to_output", dict(type=str, default="model_scores", help="directory for model_scores.csv and residue_deviation.csv")),
    ("--lddt", dict(action="store_true",
                    help="also write model_lddt.csv and residue_lddt.csv: the lDDT of every model and residue (CA atoms, thresholds 0.5, 1, 2, 4), "
                         "a superposition-free score, beside the model's B-factor (AlphaFold2's pLDDT).  PARITY UNPINNED AGAINST OPENSTRUCTURE")),
    ("--lddt_radius", dict(type=float, default=15.0, help="inclusion radius of --lddt in the reference structure (default 15.0)")),
    ("--tmscore", dict(action="store_true",
                       help="also write model_tmscore.csv: the TM-score of every model (CA atoms, normalised by the reference's length), the "
                            "maximum over superpositions found by a search on the GPU, beside the same sum under the one global fit.  At most "
                            "4096 positions per pair.  PARITY UNPINNED AGAINST THE TM-score PROGRAM")),
    ("--tm_rounds", dict(type=int, default=20, help="refinement rounds per seed of --tmscore at most (default 20)")),
    ("--cealign", dict(action="store_true",
                       help="also write model_cealign.csv and residue_cealign.csv: the sequence-independent structural alignment (CE) of the CA "
                            "atoms of every model on its native, of any two lengths (at most 2048 positions each), and the RMSD over the aligned "
                            "positions.  PARITY UNPINNED AGAINST PYMOL")),
    ("--ce_d0", dict(type=float, default=3.0, help="--cealign: two fragments of 8 are similar below this mean distance difference (default 3.0)")),
    ("--ce_d1", dict(type=float, default=4.0, help="--cealign: a path grows while its step cost and its score stay below this (default 4.0)")),
    ("--ce_gap_max", dict(type=int, default=30, help="--cealign: the longest gap between two aligned fragments, 0 .. 31 (default 30)")),
    ("--pair_by_cealign", dict(action="store_true",
                               help="pair the positions of model_scores.csv, --lddt and --tmscore by the alignment of --cealign in place of "
                                    "--pair_by: a length mismatch is then no error")),
    ("--secondary_structure", dict(action="store_true",
                                   help="also write model_secstruct.csv and residue_secstruct.csv: the DSSP class of every residue of both "
                                        "structures, the share of paired positions whose class (q8) and whose helix / strand / coil state (q3) "
                                        "agree, and the helix and strand fractions and hydrogen bonds of either side.  PARITY UNPINNED AGAINST "
                                        "DSSP")),
    # absent from the namespace unless given: a namespace built by an older caller has no such attribute either
    ("--sasa", dict(default=argparse.SUPPRESS, action="store_true",
                    help="also write model_sasa.csv and residue_sasa.csv: the solvent-accessible surface area (Shrake & Rupley) of both "
                         "structures, the share of paired positions in the same burial class, the mean absolute difference and the "
                         "correlation of their relative accessibilities.  PARITY UNPINNED AGAINST FREESASA / NACCESS / DSSP / BIOPYTHON")),
    ("--sasa_points", dict(default=argparse.SUPPRESS, type=int, help="--sasa: golden-spiral points per atom, 1 .. 1024 (default 96)")),
    ("--sasa_probe", dict(default=argparse.SUPPRESS, type=float, help="--sasa: probe radius in Angstrom (default 1.4; 0: the van der Waals surface)")),
    ("--rsa_core", dict(default=argparse.SUPPRESS, type=float, help="--sasa: a residue is core below this relative accessibility (default 0.2)")),
    ("--rsa_surface", dict(default=argparse.SUPPRESS, type=float, help="--sasa: a residue is surface from this relative accessibility (default 0.5)")),
    ("--lddt_all_atom", dict(default=argparse.SUPPRESS, action="store_true",
                             help="also write model_lddt_all_atom.csv and residue_lddt_all_atom.csv: the lDDT over all heavy atoms of the paired "
                                  "residues, with the names of symmetric side-chain atoms resolved per residue, beside its backbone and "
                                  "side-chain parts.  PARITY UNPINNED AGAINST OPENSTRUCTURE")),
    ("--lddt_no_symmetry", dict(default=argparse.SUPPRESS, action="store_true",
                                help="--lddt_all_atom: score the model as named, a flipped ring or carboxylate included")),
    ("--seqalign", dict(default=argparse.SUPPRESS, action="store_true",
                        help="also write model_seqalign.csv and residue_seqalign.csv: the sequence alignment of every model to its native "
                             "(global, affine gaps, 2 x BLOSUM62, at most 4096 residues each), its score, identity, gaps and coverage.  "
                             "PARITY UNPINNED AGAINST PYMOL")),
    ("--pair_by_seqalign", dict(default=argparse.SUPPRESS, action="store_true",
                                help="pair the positions of model_scores.csv and of every optional score by the alignment of --seqalign in "
                                     "place of --pair_by: renumbering, a missing loop and a tag are then no error.  Not with --pair_by_cealign")),
    ("--sa_gap_open", dict(default=argparse.SUPPRESS, type=float, help="--seqalign: the cost of a gap's first residue in BLOSUM62 units "
                                                                       "(default 10, cmd.align's; twice it must be an integer)")),
    ("--sa_gap_extend", dict(default=argparse.SUPPRESS, type=float, help="--seqalign: the cost of every further residue of a gap (default 0.5, "
                                                                         "cmd.align's; twice it must be an integer)")),
    ("--sa_global", dict(default=argparse.SUPPRESS, action="store_true",
                         help="--seqalign: charge the unpaired residues at either end too (default: the ends are free)")),
)


def build_parser():
    parser = argparse.ArgumentParser(description="RMSD, GDT and per-residue deviation of models superposed on their native, batched on the "
                                                 "GPU (MI355X).  PARITY UNPINNED AGAINST PYMOL; pairing by position or number, or by an alignment on request",
                                     epilog=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for flag, keywords in CLI_FLAGS:
        parser.add_argument(flag, **keywords)
    return parser


if __name__ == "__main__":
    main(build_parser().parse_args())
