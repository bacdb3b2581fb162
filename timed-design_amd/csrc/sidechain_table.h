// The side-chain topology of th_build_sidechains (sidechains.hip): for each of the 20 residue types, in the codec's order, its
// side-chain heavy atoms in BUILD ORDER, each with three parents a, b, c (d is bonded to c), the bond length |cd| in Angstrom, the
// bond angle b-c-d in degrees and the dihedral a-b-c-d in degrees: chi[k] + offset when k is 0..3, the offset alone when k is -1.
// This is the only place the tree is written down: th_sidechain_table hands it to Python, the kernels read a packed copy of it from
// constant memory.
//
//     *** PARITY UNPINNED AGAINST SCWRL4 ***  The reference places side chains with SCWRL4, which is not available where this
//     project is built.  The tree and its values are this project's own: standard stereochemistry (Engh & Huber 1991) for bond
//     lengths and angles, planar rings and carboxylates / amides / guanidinium at 0 / 180 degrees, and the offsets of the sp3
//     branches (CB, the second gamma or delta atom) from the means over 1ubq.  tests/golden/make_sidechain_golden.py prints every
//     row beside 1ubq's mean and spread and rebuilds 1ubq from its native chi angles (0.347 Angstrom RMSD over 297 atoms; the
//     per-type means of 1ubq itself give 0.331).  CYS and TRP do not occur in 1ubq: their rows are standard values, and every ring
//     is checked by the bonds in `closure`, which the tree never uses.
//
// Parents are numbered as the lanes of k_build_sidechains: 0 = N, 1 = CA, 2 = C, 3 + j = side-chain atom j of the same residue;
// a parent always comes earlier than its child.  CB is atom 0 of every type but GLY, hung on (C, N, CA): it is always built, never
// copied, so a backbone-only model and a mutated position work the same way.  After CB come the chi-path atoms of th_rotamer_table
// (path atom p[k + 3] on p[k], p[k + 1], p[k + 2] at chi[k]), then the branches.
#pragma once

constexpr int kScTypes = 20, kScMaxAtoms = 10, kScMaxClosure = 2;

struct ScRow { const char* name; signed char a, b, c, k; double length, angle, offset; };
struct ScClosure { signed char a, b; double length; };        // side-chain atom indices (not lanes) of a bond the tree does not use
struct ScType { const char* res; int n; ScRow row[kScMaxAtoms]; int n_closure; ScClosure closure[kScMaxClosure]; };

#define SC_CB {"CB", 2, 0, 1, -1, 1.530, 110.5, -122.5}

const ScType kSidechains[kScTypes] = {
    {"ALA", 1, {SC_CB}, 0, {}},
    {"CYS", 2, {SC_CB, {"SG", 0, 1, 3, 0, 1.808, 114.4, 0.0}}, 0, {}},
    {"ASP", 4, {SC_CB, {"CG", 0, 1, 3, 0, 1.516, 112.6, 0.0}, {"OD1", 1, 3, 4, 1, 1.249, 118.4, 0.0}, {"OD2", 1, 3, 4, 1, 1.249, 118.4, 180.0}}, 0, {}},
    {"GLU", 5, {SC_CB, {"CG", 0, 1, 3, 0, 1.520, 114.1, 0.0}, {"CD", 1, 3, 4, 1, 1.516, 112.6, 0.0}, {"OE1", 3, 4, 5, 2, 1.249, 118.4, 0.0},
                {"OE2", 3, 4, 5, 2, 1.249, 118.4, 180.0}}, 0, {}},
    {"PHE", 7, {SC_CB, {"CG", 0, 1, 3, 0, 1.502, 113.8, 0.0}, {"CD1", 1, 3, 4, 1, 1.384, 120.7, 0.0}, {"CD2", 1, 3, 4, 1, 1.384, 120.7, 180.0},
                {"CE1", 3, 4, 5, -1, 1.382, 120.7, 180.0}, {"CE2", 3, 4, 6, -1, 1.382, 120.7, 180.0}, {"CZ", 4, 5, 7, -1, 1.382, 120.0, 0.0}},
     1, {{5, 6, 1.382}}},
    {"GLY", 0, {}, 0, {}},
    {"HIS", 6, {SC_CB, {"CG", 0, 1, 3, 0, 1.497, 113.8, 0.0}, {"ND1", 1, 3, 4, 1, 1.378, 122.7, 0.0}, {"CD2", 1, 3, 4, 1, 1.354, 131.2, 180.0},
                {"CE1", 3, 4, 5, -1, 1.321, 109.0, 180.0}, {"NE2", 3, 4, 6, -1, 1.374, 107.2, 180.0}},
     1, {{4, 5, 1.321}}},
    {"ILE", 4, {SC_CB, {"CG1", 0, 1, 3, 0, 1.530, 110.4, 0.0}, {"CD1", 1, 3, 4, 1, 1.513, 113.8, 0.0}, {"CG2", 0, 1, 3, 0, 1.521, 110.5, -124.0}}, 0, {}},
    {"LYS", 5, {SC_CB, {"CG", 0, 1, 3, 0, 1.520, 114.1, 0.0}, {"CD", 1, 3, 4, 1, 1.520, 111.3, 0.0}, {"CE", 3, 4, 5, 2, 1.520, 111.3, 0.0},
                {"NZ", 4, 5, 6, 3, 1.489, 111.9, 0.0}}, 0, {}},
    {"LEU", 4, {SC_CB, {"CG", 0, 1, 3, 0, 1.530, 116.3, 0.0}, {"CD1", 1, 3, 4, 1, 1.521, 110.7, 0.0}, {"CD2", 1, 3, 4, 1, 1.521, 110.7, 122.0}}, 0, {}},
    {"MET", 4, {SC_CB, {"CG", 0, 1, 3, 0, 1.520, 114.1, 0.0}, {"SD", 1, 3, 4, 1, 1.803, 112.7, 0.0}, {"CE", 3, 4, 5, 2, 1.791, 100.9, 0.0}}, 0, {}},
    {"ASN", 4, {SC_CB, {"CG", 0, 1, 3, 0, 1.516, 112.6, 0.0}, {"OD1", 1, 3, 4, 1, 1.231, 120.8, 0.0}, {"ND2", 1, 3, 4, 1, 1.328, 116.4, 180.0}}, 0, {}},
    {"PRO", 3, {SC_CB, {"CG", 0, 1, 3, 0, 1.492, 104.5, 0.0}, {"CD", 1, 3, 4, 1, 1.503, 106.1, 0.0}}, 0, {}},
    {"GLN", 5, {SC_CB, {"CG", 0, 1, 3, 0, 1.520, 114.1, 0.0}, {"CD", 1, 3, 4, 1, 1.516, 112.6, 0.0}, {"OE1", 3, 4, 5, 2, 1.231, 120.8, 0.0},
                {"NE2", 3, 4, 5, 2, 1.328, 116.4, 180.0}}, 0, {}},
    {"ARG", 7, {SC_CB, {"CG", 0, 1, 3, 0, 1.520, 114.1, 0.0}, {"CD", 1, 3, 4, 1, 1.520, 111.3, 0.0}, {"NE", 3, 4, 5, 2, 1.460, 112.0, 0.0},
                {"CZ", 4, 5, 6, 3, 1.329, 124.2, 0.0}, {"NH1", 5, 6, 7, -1, 1.326, 120.0, 0.0}, {"NH2", 5, 6, 7, -1, 1.326, 120.0, 180.0}}, 0, {}},
    {"SER", 2, {SC_CB, {"OG", 0, 1, 3, 0, 1.417, 111.1, 0.0}}, 0, {}},
    {"THR", 3, {SC_CB, {"OG1", 0, 1, 3, 0, 1.433, 109.6, 0.0}, {"CG2", 0, 1, 3, 0, 1.521, 110.5, -120.5}}, 0, {}},
    {"VAL", 3, {SC_CB, {"CG1", 0, 1, 3, 0, 1.521, 110.5, 0.0}, {"CG2", 0, 1, 3, 0, 1.521, 110.5, 123.0}}, 0, {}},
    {"TRP", 10, {SC_CB, {"CG", 0, 1, 3, 0, 1.498, 113.6, 0.0}, {"CD1", 1, 3, 4, 1, 1.365, 126.9, 0.0}, {"CD2", 1, 3, 4, 1, 1.433, 126.8, 180.0},
                 {"NE1", 3, 4, 5, -1, 1.374, 110.2, 180.0}, {"CE2", 3, 4, 6, -1, 1.409, 107.2, 180.0}, {"CE3", 3, 4, 6, -1, 1.398, 133.9, 0.0},
                 {"CZ2", 4, 6, 8, -1, 1.394, 122.4, 180.0}, {"CZ3", 4, 6, 9, -1, 1.382, 118.6, 180.0}, {"CH2", 6, 8, 10, -1, 1.368, 117.5, 0.0}},
     2, {{4, 5, 1.370}, {8, 9, 1.400}}},
    {"TYR", 8, {SC_CB, {"CG", 0, 1, 3, 0, 1.512, 113.9, 0.0}, {"CD1", 1, 3, 4, 1, 1.389, 120.8, 0.0}, {"CD2", 1, 3, 4, 1, 1.389, 120.8, 180.0},
                {"CE1", 3, 4, 5, -1, 1.382, 121.2, 180.0}, {"CE2", 3, 4, 6, -1, 1.382, 121.2, 180.0}, {"CZ", 4, 5, 7, -1, 1.378, 119.6, 0.0},
                {"OH", 5, 7, 9, -1, 1.376, 119.9, 180.0}}, 1, {{5, 6, 1.378}}},
};

#undef SC_CB
