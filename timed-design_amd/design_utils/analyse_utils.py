"""calculate_seq_metrics — the one function of the reference's analyse_utils on the sampler path
(reference design_utils/analyse_utils.py:351-371; called per drawn sequence at
sampling_utils.py:132, where it dominates wall time — SURVEY.md §8 row f-2).

    *** PARITY UNPINNED ***  The reference delegates to ampal==1.5.1
    (sequence_charge, sequence_isoelectric_point, sequence_molecular_weight,
    sequence_molar_extinction_280), which is absent from /root/reference and from this image, and no
    reference test covers it.  When ampal is importable its functions are used verbatim.  Otherwise
    the restatement below (ampal's published algorithm: Henderson-Hasselbalch partial charges at
    pH 7.4 incl. termini, pI = pH of minimum |charge| on a 0.1 grid over [1,13), average residue
    masses + one water, Trp/Tyr/Cys extinction at 280 nm) is used with tabulated constants;
    ``METRICS_SOURCE`` says which.  Vectorised over a batch of sequences via residue histograms.
"""
from __future__ import annotations

import math
import typing as t

import numpy as np

_AA = "ACDEFGHIKLMNPQRSTVWY"
_MWT = dict(A=71.0779, C=103.1429, D=115.0874, E=129.114, F=147.1739, G=57.0513, H=137.1393, I=113.1576, K=128.1723,
            L=113.1576, M=131.1961, N=114.1026, P=97.1152, Q=128.1292, R=156.1857, S=87.0773, T=101.1039, V=99.1311,
            W=186.2099, Y=163.1733)
_WATER = 18.01528
_EXT280 = dict(W=5690, Y=1280, C=120)
_CHARGE = dict(C=-1, D=-1, E=-1, H=+1, K=+1, R=+1, Y=-1)
_CHARGE_TERM = {"N-term": +1, "C-term": -1}
_PKA = dict(C=8.3, D=3.65, E=4.25, H=6.1, K=10.53, R=12.48, Y=10.1)
_PKA_TERM = {"N-term": 8.0, "C-term": 3.1}

try:  # pragma: no cover - ampal is not installed in the build image
    from ampal.analyse_protein import (sequence_charge, sequence_isoelectric_point, sequence_molar_extinction_280,
                                       sequence_molecular_weight)
    METRICS_SOURCE = "ampal"
except Exception:  # ImportError or a broken optional dependency
    METRICS_SOURCE = "restatement (unpinned)"
    sequence_charge = None


def _partial(pka: float, sign: int, ph) -> np.ndarray:
    """ampal's partial_charge: 10**d / (1 + 10**d), d = pH - pKa (negated for basic groups).  ampal evaluates it with
    Python floats, i.e. libm pow — so does this (NumPy's vectorised power may round differently) and so does the table
    the device kernel uses (csrc/sampler.hip build_metric_tables)."""
    out = []
    for p in np.atleast_1d(np.asarray(ph, dtype=float)):
        diff = float(p) - pka
        if sign > 0:
            diff = -diff
        r = math.pow(10.0, diff)
        out.append(r / (1.0 + r))
    return np.array(out)


def _charge_table(ph) -> t.Tuple[np.ndarray, np.ndarray]:
    """signed partial charge of one residue of each class (alphabetical order) and of the two termini at each pH"""
    ph = np.atleast_1d(np.asarray(ph, dtype=float))
    per_res = np.zeros((20, ph.size))
    for aa, sign in _CHARGE.items():
        per_res[_AA.index(aa)] = _partial(_PKA[aa], sign, ph) * sign
    term = _partial(_PKA_TERM["N-term"], +1, ph) * (+1) + _partial(_PKA_TERM["C-term"], -1, ph) * (-1)
    return per_res, term


def _dot_in_class_order(counts: np.ndarray, table: np.ndarray) -> np.ndarray:
    """sum_c counts[:, c] * table[c] accumulated strictly in class order (c = 0..19) — the order the device kernel
    (csrc/sampler.hip k_seq_metrics) uses, so that the two agree bit for bit (a BLAS dot would not)."""
    acc = np.zeros((counts.shape[0],) + table.shape[1:])
    for c in range(20):
        acc = acc + counts[:, c].reshape((-1,) + (1,) * (table.ndim - 1)) * table[c]
    return acc


def _charge_from_counts(counts: np.ndarray, ph) -> np.ndarray:
    """counts [n_seq, 20] -> net charge [n_seq, len(ph)]"""
    per_res, term = _charge_table(ph)
    return _dot_in_class_order(counts, per_res) + term[None, :]


def residue_counts(seqs: t.Sequence[str]) -> np.ndarray:
    lut = np.full(256, -1, dtype=np.int64)
    for i, a in enumerate(_AA):
        lut[ord(a)] = i
    counts = np.zeros((len(seqs), 20))
    for k, s in enumerate(seqs):
        idx = lut[np.frombuffer(s.encode("ascii"), dtype=np.uint8)]
        counts[k] = np.bincount(idx[idx >= 0], minlength=20)
    return counts


def seq_metrics_batch(seqs: t.Sequence[str]) -> np.ndarray:
    """[n_seq, 4] = (charge at pH 7.4, isoelectric point, molecular weight, molar extinction at 280)."""
    if sequence_charge is not None:  # pragma: no cover
        return np.array([[sequence_charge(s), sequence_isoelectric_point(s), sequence_molecular_weight(s),
                          sequence_molar_extinction_280(s)] for s in seqs], dtype=float)
    counts = residue_counts(seqs)
    grid = np.arange(1, 13, 0.1)                # NumPy fills first + i*((1 + 0.1) - 1): 120 points
    charge = _charge_from_counts(counts, [7.4])[:, 0]
    pi = grid[np.abs(_charge_from_counts(counts, grid)).argmin(axis=1)]
    mw = _dot_in_class_order(counts, np.array([_MWT[a] for a in _AA])) + _WATER
    ext = _dot_in_class_order(counts, np.array([float(_EXT280.get(a, 0)) for a in _AA]))
    return np.stack([charge, pi, mw, ext], axis=1)


def calculate_seq_metrics(seq: str) -> t.Tuple[float, float, float, float]:
    """reference analyse_utils.py:351-371 -> (charge, iso_ph, mw, me)."""
    c, p, m, e = seq_metrics_batch([seq])[0]
    return float(c), float(p), float(m), int(e) if float(e).is_integer() else float(e)


# ---- prediction entropy (predict.py --output_analysis; computed on the GPU by timed_hip.analysis) -----------------------------
def calculate_prediction_entropy(residue_predictions) -> np.ndarray:
    """reference analyse_utils.py:294-310: Shannon entropy in bits of every row of an (n, k) probability matrix —
    ``scipy.stats.entropy(residue_predictions, base=2, axis=1)`` — computed by th_analyse_probs.  Differs from scipy for a row
    with a negative entry (NaN here, -inf there); float64 rows are narrowed as timed_hip.analysis.entropy says."""
    from timed_hip import analysis
    return analysis.entropy(np.asarray(residue_predictions))


def extract_prediction_entropy_to_dict(model_pred_path, model_map_path, rotamer_mode: bool = False, is_old: bool = False) -> dict:
    """reference analyse_utils.py:237-291: {key: entropy of each of its rows} for a prediction CSV and its dataset map (key and
    row order as extract_sequence_from_pred_matrix gives them).  ``rotamer_mode`` names a 338-column matrix (``<model>_rot.csv``);
    the entropy is over all of its columns either way."""
    from pathlib import Path

    from . import utils
    model_pred_path, model_map_path = Path(model_pred_path), Path(model_map_path)
    assert model_pred_path.exists(), f"Model path {model_pred_path} does not exists."
    assert model_map_path.exists(), f"Model path {model_map_path} does not exists."
    prediction_matrix = np.atleast_2d(np.loadtxt(model_pred_path, delimiter=",", dtype=np.float64))
    if rotamer_mode and prediction_matrix.shape[1] != 338:
        raise ValueError(f"rotamer_mode expects 338 columns, {model_pred_path} has {prediction_matrix.shape[1]}")
    plan = utils.SequencePlan(utils.load_datasetmap(model_map_path, is_old=is_old))
    entropy = calculate_prediction_entropy(prediction_matrix)
    return {key: entropy[plan.rows(key)] for key in plan.keys}


# ---- structure properties (analyse_properties.py; packing density computed on the GPU by timed_hip.structure) -----------------
def extract_packdensity_from_ampal(pdb, load_pdb: bool = True, atom_filter: str = "ca", radius: float = 7.0, device: int = 0) -> t.List[t.List[float]]:
    """reference analyse_utils.py:204-234: ``[[packing density of each residue of the first chain]]`` — the atomic contact number
    within ``radius`` (the reference always uses 7) summarised per residue with the reference's running half-average over the
    atoms ``atom_filter`` selects ("ca": atoms named C and CA, the reference's substring test; "backbone"; "all"; "calpha" is
    an addition).  ``pdb`` is a path (plain or gzipped PDB file) or, with ``load_pdb=False``, a ``timed_hip.pdbio.Model`` — where
    the reference takes an ampal Assembly.  The object model differs from ampal's: which atoms are neighbours and which residues
    are reported is the structure rule written out in timed_hip/structure.py (first model, all non-hydrogen ATOM and HETATM atoms
    as neighbours, the non-hetero residues of the first chain reported), unpinned against ampal; the arithmetic is the
    reference's, bit for bit.  Values are floats where the reference mixes NumPy integers and floats."""
    from timed_hip import structure
    model = structure.first_model(pdb) if load_pdb else pdb
    res = structure.packing_density([model], radius=radius, atom_filter=atom_filter, device=device)[0]
    return [[float(v) for v in res.residue_density]]


def extract_sasa_from_ampal(pdb, load_pdb: bool = True, probe: float = 1.4, n_points: int = 96, include_hetero: bool = False,
                            device: int = 0) -> t.List[t.List[float]]:
    """No counterpart in the reference, named after its siblings: one list per chain (non-hetero residues, chains in order of
    appearance) with the solvent-accessible surface area of each residue in square Angstrom — Shrake & Rupley (1973) with
    ``n_points`` golden-spiral points per atom, element radii after Bondi plus ``probe``, on the GPU through
    ``timed_hip.sasa.sasa``.  ``pdb`` is a path (plain or gzipped PDB file) or, with ``load_pdb=False``, a ``timed_hip.pdbio.Model``.
    PARITY UNPINNED AGAINST FREESASA / NACCESS / DSSP / BIOPYTHON: the rule is this project's own (include/timed_hip.h, th_sasa).
    For many structures call ``sasa`` itself: it batches them."""
    from timed_hip import sasa, structure
    model = structure.first_model(pdb) if load_pdb else pdb
    (res,) = sasa.sasa([model], probe=probe, n_points=n_points, include_hetero=include_hetero, device=device)
    chains: dict = {}
    for r, a in zip(res.residues, res.residue_area.tolist()):
        chains.setdefault(r.chain, []).append(float(a))
    return list(chains.values())


def calculate_sequence_identity(real_seq: str, predicted_seq: str, device: int = 0) -> float:
    """The reference's "Sequence Identity" (ui.py, ``accuracy_score(list(seq), list(native))``): the share of positions at which the two
    equally long sequences hold the same letter, on the GPU through ``timed_hip.seqset``.  For many sequences call
    ``timed_hip.seqset.analyse`` itself: it scores whole sets in one call."""
    from timed_hip import seqset
    return seqset.identity_and_similarity(real_seq, predicted_seq, device=device)[0]


def calculate_sequence_similarity(real_seq: str, predicted_seq: str, device: int = 0) -> float:
    """The reference's "Sequence Similarity" (ui.py ``_calculate_sequence_similarity_wrapper``): the share of positions with
    ``lookup_blosum62(a, b) > 0``, over the positions at which both letters are among the twenty (the reference's lookup is defined
    only there; NaN when there is none), on the GPU through ``timed_hip.seqset``."""
    from timed_hip import seqset
    return seqset.identity_and_similarity(real_seq, predicted_seq, device=device)[1]


def extract_bfactor_from_ampal(pdb_path, load_pdb: bool = True) -> t.List[t.List[float]]:
    """reference analyse_utils.py:112-146: one list per chain with the B-factor of the first atom of each residue (AlphaFold2
    models carry the pLDDT there).  ``pdb_path`` is a path or, with ``load_pdb=False``, a ``timed_hip.pdbio.Model``.  Differs
    from ampal's object model: chains are the chain identifiers of the first model's ATOM records in file order (ampal splits
    polypeptides by its own rules and skips ligands and nucleic acids); a missing B-factor column reads as NaN.  Host code."""
    from timed_hip import structure
    model = structure.first_model(pdb_path) if load_pdb else pdb_path
    return structure.residue_bfactors(model)


def calculate_RMSD_and_gdt(pdb_original_path, pdb_predicted_path, device: int = 0) -> t.Tuple[float, float]:
    """reference scripts/analyse_af2.py:12-45: ``(rmsd, mean_gdt)`` of a predicted structure on its original — there PyMOL's
    ``cmd.align`` on the CA atoms and the mean of the fractions of aligned pairs within 1, 2, 4 and 8 Angstrom.  Here
    ``(rmsd_kept, mean_gdt)`` of ``timed_hip.superpose.superpose`` with the CA atoms paired by position, ``cycles=5``,
    ``cutoff=2.0``: PARITY UNPINNED AGAINST PYMOL, the rule is this project's reading of cmd.align's documented behaviour
    (include/timed_hip.h, th_superpose) and no sequence alignment is made.  Structures of different length raise ValueError, where
    the reference's callers assert equal length beforehand.  For many pairs call ``superpose`` itself: it batches them."""
    from timed_hip import superpose
    (res,) = superpose.superpose([(pdb_original_path, pdb_predicted_path)], device=device)
    if res.error:
        raise ValueError(f"{pdb_original_path} / {pdb_predicted_path}: {res.error}")
    return res.rmsd_kept, res.mean_gdt


def calculate_cealign_RMSD(pdb_original_path, pdb_predicted_path, device: int = 0) -> float:
    """reference scripts/analyse_all_properties.py:23-34 ``_calculate_RMSD`` (and ``calculate_RMSD_and_gdt`` of
    scripts/analyse_cherrypicked_samples_af2.py): the RMSD of a predicted structure on its original after PyMOL's ``cmd.cealign`` on
    the CA atoms — a sequence-independent structural alignment, so the two files need be neither equally long nor numbered alike.
    Here the ``rmsd`` of ``timed_hip.cealign.cealign`` with cealign's defaults (window 8, d0 3.0, d1 4.0, gap_max 30):
    PARITY UNPINNED AGAINST PYMOL, the rule is this project's reading of the published CE algorithm (include/timed_hip.h, th_cealign).  NaN when no
    two fragments are similar enough to align; a file that cannot be read or a structure of more than 2048 positions raises
    ValueError.  For many pairs call ``cealign`` itself: it batches them."""
    from timed_hip import cealign
    (res,) = cealign.cealign([(pdb_original_path, pdb_predicted_path)], device=device)
    if res.error:
        raise ValueError(f"{pdb_original_path} / {pdb_predicted_path}: {res.error}")
    return res.rmsd


def align_sequences(a: str, b: str, device: int = 0) -> t.Tuple[str, str, int]:
    """The sequence alignment of two strings of one-letter codes, ``a`` the reference: the two sequences written over one another
    with ``-`` where a residue has no partner, and the score in units of the table — ``timed_hip.seqalign.align_strings`` with its
    defaults (2 x BLOSUM62, a run of k unpaired residues costs 20 + (k - 1), free ends; halve the score for BLOSUM62 units).  This
    is the alignment step of PyMOL's ``cmd.align``, which the reference's scripts/analyse_af2.py calls: PARITY UNPINNED AGAINST PYMOL,
    the rule is this project's own (include/timed_hip.h, th_seqalign).  A sequence of more than 4096 residues raises ValueError.
    For many pairs call ``align_strings`` itself: it batches them."""
    from timed_hip import seqalign
    (res,) = seqalign.align_strings([(a, b)], device=device)
    if res.error:
        raise ValueError(res.error)
    top, bottom = seqalign.gapped(str(a), str(b), res)
    return top, bottom, res.score


def calculate_all_atom_lddt(pdb_original_path, pdb_predicted_path, device: int = 0) -> float:
    """The all-atom lDDT (Mariani et al. 2013) of a predicted structure against its original, over the heavy atoms of the residues
    paired by position, with the names of symmetric side-chain atoms resolved per residue: ``lddt`` of
    ``timed_hip.lddt_atoms.lddt_atoms``.  PARITY UNPINNED AGAINST OPENSTRUCTURE: the rule is this project's reading of the published
    definition (include/timed_hip.h, th_lddt_atoms).  Structures of different length or a file that cannot be read raise ValueError.
    For many pairs call ``lddt_atoms`` itself: it batches them."""
    from timed_hip import lddt_atoms
    (res,) = lddt_atoms.lddt_atoms([(pdb_original_path, pdb_predicted_path)], device=device)
    if res.error:
        raise ValueError(f"{pdb_original_path} / {pdb_predicted_path}: {res.error}")
    return res.lddt


# ---- per-class rotamer metrics (analyse_rotamers.py; computed on the GPU by timed_hip.analysis) -------------------------------
def _narrow(matrix: np.ndarray) -> np.ndarray:
    """float16 / float32 matrices as they are; others to float16 when that is exact (the probability CSVs predict.py writes),
    else to float32"""
    if matrix.dtype in (np.float16, np.float32):
        return matrix
    a64 = matrix.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        h = a64.astype(np.float16)
    return h if np.array_equal(h.astype(np.float64), a64, equal_nan=True) else a64.astype(np.float32)


def calculate_rotamer_metrics(pdb_to_probability, pdb_to_rotamer: dict, rot_categories: t.List[str], suffix: str, output_path,
                              device: int = 0) -> dict:
    """reference analyse_utils.py:731-898: per-class metrics of a rotamer model — ROC AUC one-vs-one and one-vs-rest, the
    classification report, top-1..5 accuracy, macro precision and recall, prediction bias and the plain and label-weighted
    confusion matrices — for {key: rows of probabilities} (a dict of lists, or the lazy mapping extract_sequence_from_pred_matrix
    returns) against {key: rotamer class per residue} (NaN / None = untagged).  Same pairing rules: a key missing from
    ``pdb_to_rotamer``, or whose lengths differ, is reported on stdout and skipped.  Everything is derived from the integer
    totals of one GPU call (timed_hip.analysis.analyse_class_matrix, which documents every key and the one deliberate
    difference: the AUC is of the matrix as stored, no residual is spread over rows that do not sum to 1).

    Writes results_{suffix}.txt (the reference's line labels), results_{suffix}.json (the whole dict) and
    cm_{suffix}_unweighted.csv / cm_{suffix}_weighted.csv (k x k, np.savetxt's format) where the reference draws two PNGs.
    Returns the dict (the reference returns None)."""
    import json
    from pathlib import Path

    from timed_hip import analysis, textio
    k = len(rot_categories)
    output_path = Path(output_path)
    output_path.mkdir(parents=True, exist_ok=True)
    parts, labels = [], []
    for pdb in pdb_to_probability.keys():
        if pdb in pdb_to_rotamer:
            rows = pdb_to_probability.matrix(pdb) if hasattr(pdb_to_probability, "matrix") else \
                np.asarray(pdb_to_probability[pdb]).reshape(-1, k)
            if len(rows) == len(pdb_to_rotamer[pdb]):
                parts.append(np.asarray(rows))
                labels.append(np.array([np.nan if v is None else v for v in pdb_to_rotamer[pdb]], dtype=np.float64).reshape(-1))
            else:
                print(f"Error with pdb code {pdb} - Length Mismatch")
        else:
            print(f"Error with pdb code {pdb}")
    y_pred = np.concatenate(parts).reshape(-1, k) if parts else np.empty((0, k), np.float16)
    y_true = np.concatenate(labels) if labels else np.empty(0)
    true_class = np.where(np.isnan(y_true), -1, y_true).astype(np.int64)
    results = analysis.analyse_class_matrix(_narrow(y_pred), true_class, categories=list(rot_categories), device=device)
    print("Metrics AUC_OVR")
    print(results["auc_ovr"])
    print("Metrics AUC_OVO")
    print(results["auc_ovo"])
    print(", ".join(f"{name}: {results[key]}" for name, key in (
        ("Accuracy", "accuracy_1"), ("accuracy_2", "accuracy_2"), ("accuracy_3", "accuracy_3"), ("accuracy_4", "accuracy_4"),
        ("accuracy_5", "accuracy_5"), ("precision", "precision"), ("recall", "recall"))))
    with open(output_path / f"results_{suffix}.txt", "w") as f:
        f.write(f"Metrics AUC_OVR: {results['auc_ovr']}\n")
        f.write(f"Metrics AUC_OVO: {results['auc_ovo']}\n")
        f.write(f"Metrics AUC_OVR (classes present): {results['auc_ovr_present']}\n")
        f.write(f"Metrics Macro-Precision: {results['precision']}\n")
        f.write(f"Metrics Macro-Recall: {results['recall']}\n")
        f.write(f"Accuracy: {results['accuracy_1']}\n")
        for kk in range(2, 6):
            f.write(f"accuracy_{kk}: {results[f'accuracy_{kk}']}\n")
        f.write(f"precision: {results['precision']}\nrecall: {results['recall']}\n")
        f.write("Report:\n")
        f.write(f"{results['report']}\n")
        f.write("Bias:\n")
        f.write(f"{results['bias']}\n")
    with open(output_path / f"results_{suffix}.json", "w") as f:
        json.dump(results, f, indent=1, allow_nan=False)
        f.write("\n")
    for kind in ("unweighted", "weighted"):
        cm = np.zeros((k, k)) if results[f"{kind}_cm"] is None else np.array(results[f"{kind}_cm"], dtype=np.float64)
        with open(output_path / f"cm_{suffix}_{kind}.csv", "wb") as f:
            f.write(textio.format_csv(cm))
    return results


# ---- rotamer labels from structures (analyse_rotamers.py, tag_rotamers.py; computed on the GPU by timed_hip.structure) ----------
class RotamerChain:
    """One chain of a tagged structure — what the reference iterates as an ampal Polypeptide: ``id``, ``sequence`` (one letter
    per residue, X for a residue that is not one of the 20), ``residues`` (timed_hip.pdbio.Residue) and ``classes`` (rotamer class
    per residue, -1 where unlabelled)."""

    def __init__(self, chain_id: str, residues: list, classes: np.ndarray):
        from .amino_acids import standard_amino_acids
        one_letter = {three: one for one, three in standard_amino_acids.items()}
        self.id, self.residues, self.classes = chain_id, residues, np.asarray(classes)
        self.sequence = "".join(one_letter.get(r.name, "X") for r in residues)

    def __len__(self):
        return len(self.residues)


def chains_of(tagged) -> t.Dict[str, RotamerChain]:
    """{chain id: RotamerChain} of one timed_hip.structure.StructureRotamers, chains in file order"""
    members: t.Dict[str, t.List[int]] = {}
    for k, r in enumerate(tagged.residues):
        members.setdefault(r.chain, []).append(k)
    return {cid: RotamerChain(cid, [tagged.residues[k] for k in idx], tagged.cls[idx]) for cid, idx in members.items()}


def extract_rotamer_encoding(pdb_code: str, monomer: RotamerChain) -> dict:
    """reference analyse_utils.py:901-930: ``{pdb_code[:4] + chain id: [rotamer class or nan per residue]}`` for one tagged chain
    (a RotamerChain where the reference takes an ampal Polypeptide that went through tag_sidechain_dihedrals)."""
    return {f"{pdb_code[:4]}{monomer.id}": [float("nan") if c < 0 else int(c) for c in monomer.classes.tolist()]}


def rotamer_structure_path(path_to_pdb, pdb_code: str):
    """The reference's file rule (analyse_utils.py:951-963): a code with ``_`` is ``<path>/<code>.pdb``; any other is
    ``<path>/<code[1:3]>/<code[:4]>.pdb1.gz``, then ``.pdb1``.  Returns (the file or None, the last path tried).  Nothing is
    created and nothing is ever fetched (the reference downloads a missing biological unit)."""
    from pathlib import Path
    path_to_pdb = Path(path_to_pdb)
    if "_" in pdb_code:
        tried = [path_to_pdb / (pdb_code + ".pdb")]
    else:
        tried = [path_to_pdb / pdb_code[1:3] / (pdb_code[:4] + suffix) for suffix in (".pdb1.gz", ".pdb1")]
    for candidate in tried:
        if candidate.exists():
            return candidate, candidate
    return None, tried[-1]


def tag_pdb_with_rot(workers: int, path_to_pdb, pdb_codes, device: int = 0) -> t.Tuple[dict, dict]:
    """reference analyse_utils.py:933-1036: ``(results_dict, pdb_to_assemblies)`` for the structures of ``pdb_codes`` under
    ``path_to_pdb`` (file rule: rotamer_structure_path; a missing file prints ``Could not find ...`` and is skipped).
    ``results_dict`` is {pdb4 + chain: [rotamer class or nan per residue]}, ``pdb_to_assemblies`` {pdb4: {chain: RotamerChain}} —
    ``pdb_to_assemblies[pdb4][chain].sequence`` is what the reference reads from it.  The files are parsed on ``workers`` host
    threads (at most 16) and ALL structures are tagged on the GPU together (timed_hip.structure.tag_rotamers; the rule is this
    project's own, PARITY UNPINNED AGAINST AMPAL, see timed_hip/structure.py)."""
    from timed_hip import batching, structure
    found = []
    for code in pdb_codes:
        code = str(code)
        path, tried = rotamer_structure_path(path_to_pdb, code)
        if path is None:
            print(f"Could not find {tried}")
        else:
            found.append((code, path))
    layouts = batching.parse_each(lambda item: structure.rotamer_layout(structure.first_model(item[1])), found, workers)
    results_dict, pdb_to_assemblies = {}, {}
    for (code, _), tagged in zip(found, structure.tag_rotamers(layouts, device=device)):
        chains = chains_of(tagged)
        for monomer in chains.values():
            results_dict.update(extract_rotamer_encoding(code, monomer))
        pdb_to_assemblies[code[:4]] = chains
    return results_dict, pdb_to_assemblies


def rotamer_labels_json(results_dict: dict) -> dict:
    """{key: [class or None]}: the labels file analyse_rotamers.py reads (--path_to_rotamer_labels) from a results_dict"""
    return {key: [None if v != v else int(v) for v in values] for key, values in results_dict.items()}


# ---- side chains packed by a rotamer search (analyse_rotamers.py --pack; computed on the GPU by timed_hip.packer) ----------------
def _types_of_sequence(sequence: str) -> np.ndarray:
    from .amino_acids import standard_amino_acids
    index = {one: k for k, one in enumerate(standard_amino_acids.keys())}
    return np.array([index.get(letter, -1) for letter in sequence], dtype=np.int8)


def _model_of_chains(chains: t.Dict[str, RotamerChain]):
    from timed_hip import pdbio
    return pdbio.Model(1, [r for chain in chains.values() for r in chain.residues])


def pack_sidechains(structure: t.Dict[str, RotamerChain], sequence, device: int = 0, **packer_keywords):
    """The place of the reference's pack_sidechains (analyse_utils.py:393-416: a structure and a sequence to SCWRL4, the packed
    structure back) — SCWRL4 IS NOT CALLED (PARITY UNPINNED AGAINST SCWRL4: it is not available where this project is built).  The
    sequence is packed onto the backbone by this project's own rotamer search, timed_hip.packer (an integer steric ladder, greedy
    sweeps from a deterministic start; no rotamer library, no SCWRL4 energy), without a prior.

    ``structure``: {chain id: RotamerChain}, an entry of tag_pdb_with_rot's ``pdb_to_assemblies``.  ``sequence``: one string of
    one-letter codes over all chains in order, or one string per chain; a letter that is not one of the 20 leaves its residue
    unbuilt.  Returns the timed_hip.packer.PackedSidechains (``.built.to_model()`` is the packed structure, ``.energy_final`` takes
    the place of the SCWRL score)."""
    from timed_hip import packer
    sequence = sequence if isinstance(sequence, str) else "".join(sequence)
    model = _model_of_chains(structure)
    if len(sequence) != len(model.residues):
        raise ValueError(f"the sequence has {len(sequence)} letters, the structure {len(model.residues)} residues")
    return packer.pack([model], types=[_types_of_sequence(sequence)], prior="none", device=device, **packer_keywords)[0]


def analyse_with_packer(pdb_to_seq: dict, pdb_to_assembly: dict, output_path, suffix: str, device: int = 0, **packer_keywords) -> t.Tuple[dict, dict]:
    """The place of the reference's analyse_with_scwrl (analyse_utils.py:419-500) — SCWRL4 IS NOT CALLED (see pack_sidechains).
    For every key ``<pdb><chain>`` of ``pdb_to_seq`` whose structure is in ``pdb_to_assembly`` ({pdb4: {chain: RotamerChain}}) the
    sequence is paired by position with the residues of that chain; a chain without a sequence, or whose sequence has another
    length (reported on stdout), keeps its native residue types, so that every chain packs against a complete neighbourhood.
    ALL structures are packed in one batch on the GPU, without a prior, and written to ``<output_path>/<pdb4><suffix>.pdb``.
    Returns ({key: final energy of the key's structure} — the counterpart of the SCWRL scores — and {pdb4: PackedSidechains})."""
    from pathlib import Path

    from timed_hip import packer, pdbio
    output_path = Path(output_path)
    output_path.mkdir(parents=True, exist_ok=True)
    codes, models, types = [], [], []
    for code in dict.fromkeys(str(key)[:4] for key in pdb_to_seq):
        if code not in pdb_to_assembly:
            print(f"Error with pdb code {code}: no structure")
            continue
        chains = pdb_to_assembly[code]
        per_chain = []
        for chain_id, chain in chains.items():
            sequence = pdb_to_seq.get(f"{code}{chain_id}")
            if sequence is not None and len(sequence) != len(chain):
                print(f"Error with pdb code {code}{chain_id} - Length Mismatch")
                sequence = None
            per_chain.append(_types_of_sequence(chain.sequence if sequence is None else sequence))
        codes.append(code)
        models.append(_model_of_chains(chains))
        types.append(np.concatenate(per_chain) if per_chain else np.zeros(0, np.int8))
    packed = packer.pack(models, types=types, prior="none", device=device, **packer_keywords)
    pdb_to_packed = dict(zip(codes, packed))
    for code, result in pdb_to_packed.items():
        pdbio.write_pdb(output_path / f"{code}{suffix}.pdb", result.built.to_model())
    pdb_to_scores = {str(key): pdb_to_packed[str(key)[:4]].energy_final for key in pdb_to_seq if str(key)[:4] in pdb_to_packed}
    return pdb_to_scores, pdb_to_packed
