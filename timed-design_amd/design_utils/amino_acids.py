"""Amino-acid tables the hot path needs (the reference takes them from ampal.amino_acids,
reference design_utils/utils.py:10-15, design_utils/sampling_utils.py:7).

``standard_amino_acids`` is ordered by one-letter code — the order that fixes the column meaning of
every probability matrix (`residue_encoder`, argmax → letter at reference utils.py:655-659) — and
``side_chain_dihedrals`` carries the number of chi angles per residue, which fixes the 338 rotamer
categories (3**n_chi per residue; reference utils.py:430-462).  With these tables
``get_rotamer_codec`` reproduces the reduction guide printed in the reference docstring
(utils.py:425) and the reference-generated fixture tests/golden/sampler_golden.npz.
"""

standard_amino_acids = {
    "A": "ALA", "C": "CYS", "D": "ASP", "E": "GLU", "F": "PHE", "G": "GLY", "H": "HIS", "I": "ILE", "K": "LYS",
    "L": "LEU", "M": "MET", "N": "ASN", "P": "PRO", "Q": "GLN", "R": "ARG", "S": "SER", "T": "THR", "V": "VAL",
    "W": "TRP", "Y": "TYR",
}

# residue -> number of side-chain dihedrals (ALA and GLY have none and get a single "_0" category)
_N_CHI = {"ARG": 4, "ASN": 2, "ASP": 2, "CYS": 1, "GLN": 3, "GLU": 3, "HIS": 2, "ILE": 2, "LEU": 2, "LYS": 4, "MET": 3,
          "PHE": 2, "PRO": 2, "SER": 1, "THR": 1, "TRP": 2, "TYR": 2, "VAL": 1}
side_chain_dihedrals = {res: list(range(n)) for res, n in _N_CHI.items()}

# ---- residue properties (the sixth frame channel of TIMED_charge / TIMED_polar; timed_hip/voxeliser.py spec item 8) ----
# PARITY UNPINNED AGAINST AMPAL AND APOSTERIORI.  The reference takes ``residue_charge`` and ``polarity_Zimmerman`` from
# ampal.amino_acids (reference design_utils/utils.py:10-15), which is not available here.  What the reference itself pins is
# only {0: "A", 1: "K", -1: "D"} (utils.py:86) and the polarity threshold of 20 (utils.py:95); both tables below agree with it.
# Whether ampal's charge table puts C and Y at -1 is a recollection, not a checked fact.
residue_charge = {
    "A": 0, "C": -1, "D": -1, "E": -1, "F": 0, "G": 0, "H": +1, "I": 0, "K": +1, "L": 0, "M": 0, "N": 0, "P": 0, "Q": 0,
    "R": +1, "S": 0, "T": 0, "V": 0, "W": 0, "Y": -1,
}
# Zimmerman, Eliezer & Simha (1968) polarity scale as commonly tabulated; only "below 20 or not" is ever used
polarity_Zimmerman = {
    "A": 0.0, "C": 1.48, "D": 49.7, "E": 49.9, "F": 0.35, "G": 0.0, "H": 51.6, "I": 0.13, "K": 49.5, "L": 0.13, "M": 1.43,
    "N": 3.38, "P": 1.58, "Q": 3.53, "R": 52.0, "S": 1.67, "T": 1.66, "V": 0.13, "W": 2.1, "Y": 1.61,
}
POLARITY_THRESHOLD = 20                  # reference utils.py:95: polar (1) iff polarity_Zimmerman >= 20
residue_polarity = {r: (0 if v < POLARITY_THRESHOLD else 1) for r, v in polarity_Zimmerman.items()}     # polar: R, D, E, H, K
PROPERTIES = ("polarity", "charge")      # the reference's accepted_properties (utils.py:82)
PROPERTY_VALUES = {"polarity": (0, 1), "charge": (-1, 0, 1)}
PROPERTY_TABLE = {"polarity": residue_polarity, "charge": residue_charge}

# Solvent-accessible surface area (timed_hip/sasa.py).  Van der Waals radii by element in Angstrom (Bondi 1964); an element that is
# not listed takes VDW_RADIUS_OTHER.  A caller may pass a dict of their own.
vdw_radii = {"C": 1.70, "N": 1.55, "O": 1.52, "S": 1.80, "P": 1.80, "SE": 1.90}
VDW_RADIUS_OTHER = 1.80
# Maximum solvent-accessible area of each residue in Angstrom^2, after Tien et al. 2013 (their theoretical values): the divisor of
# the relative accessibility.  WRITTEN FROM MEMORY, NOT FETCHED: nothing here could be checked against the paper.
max_asa = {
    "ALA": 129.0, "ARG": 274.0, "ASN": 195.0, "ASP": 193.0, "CYS": 167.0, "GLN": 225.0, "GLU": 223.0, "GLY": 104.0, "HIS": 224.0,
    "ILE": 197.0, "LEU": 201.0, "LYS": 236.0, "MET": 224.0, "PHE": 240.0, "PRO": 159.0, "SER": 155.0, "THR": 172.0, "TRP": 285.0,
    "TYR": 263.0, "VAL": 174.0,
}
WATER_NAMES = ("HOH", "WAT", "DOD")

# All-atom lDDT (timed_hip/lddt_atoms.py).  residue -> the pairs of side-chain atom names that a 180-degree turn of the last chi angle
# exchanges: the same molecule under either naming.  WRITTEN FROM MEMORY, NOT FETCHED: nothing here could be checked against
# OpenStructure's table of symmetric atoms.
SYMMETRIC_ATOMS = {
    "ASP": (("OD1", "OD2"),),
    "GLU": (("OE1", "OE2"),),
    "PHE": (("CD1", "CD2"), ("CE1", "CE2")),
    "TYR": (("CD1", "CD2"), ("CE1", "CE2")),
    "ARG": (("NH1", "NH2"),),
    "LEU": (("CD1", "CD2"),),
    "VAL": (("CG1", "CG2"),),
}

# Stand-in for aposteriori.config.UNCOMMON_RESIDUE_DICT (used at reference utils.py:381-385 to map a
# non-standard residue label onto its parent amino acid while the dataset map is built).  aposteriori
# 2.4.0 is not in the reference tree nor in this image, so its exact table is UNPINNED; this one holds
# the common modified residues of the PDB and can be extended/replaced by the caller
# (design_utils.utils.create_flat_dataset_map(..., uncommon_residue_dict=...)).
UNCOMMON_RESIDUE_DICT = {
    "MSE": "MET", "SEP": "SER", "TPO": "THR", "PTR": "TYR", "HYP": "PRO", "CSO": "CYS", "CME": "CYS", "OCS": "CYS",
    "CSD": "CYS", "CSS": "CYS", "KCX": "LYS", "LLP": "LYS", "MLY": "LYS", "M3L": "LYS", "MLZ": "LYS", "ALY": "LYS",
    "PCA": "GLU", "SEC": "CYS", "PYL": "LYS", "HIC": "HIS", "FME": "MET", "DAL": "ALA", "DAR": "ARG", "DAS": "ASP",
    "DCY": "CYS", "DGL": "GLU", "DGN": "GLN", "DHI": "HIS", "DIL": "ILE", "DLE": "LEU", "DLY": "LYS", "DPN": "PHE",
    "DPR": "PRO", "DSN": "SER", "DSG": "ASN", "DTH": "THR", "DTR": "TRP", "DTY": "TYR", "DVA": "VAL",
}
