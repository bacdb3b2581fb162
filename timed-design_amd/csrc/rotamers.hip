// th_tag_rotamers: side-chain dihedrals (chi angles) and rotamer classes of every residue of a BATCH of structures — what the
// reference gets per structure from ampal (design_utils/analyse_utils.py tag_pdb_with_rot / extract_rotamer_encoding :901-1036:
// ``monomer.tag_sidechain_dihedrals()``, then a lookup of "<RES>_<bins>" in the 338 categories of get_rotamer_codec).
//
//     *** PARITY UNPINNED AGAINST AMPAL ***  ampal is neither in the reference tree nor installed where this project is built.  The
//     atom paths, the bin edges (bin 1: 0 <= chi < 120, bin 3: -120 <= chi < 0, bin 2: the rest) and the ALA / GLY rule below are
//     this project's reading of ampal 1.5's classify_angle_as_rotamer / tag_sidechain_dihedrals, written out in include/timed_hip.h.
//
// Every chi angle of every residue is a window of four consecutive atoms on ONE path of n_chi + 3 atoms: N, CA, CB and the tail of
// kRotamers below; chi k is the dihedral of path[k .. k + 3].  That table is the only place the paths are written down:
// th_rotamer_table hands it to Python, the kernel receives it by value.
//
// k_tag_rotamers: eight lanes per residue, 32 residues per workgroup.  Lane p < n_chi + 3 scans the residue's own atoms, in file
// order, for path name p (names are four packed ASCII bytes, one integer compare; the first atom with the name wins) and keeps
// its coordinates; lane k < n_chi then takes the three atoms after its own from lanes k + 1 .. k + 3 by shuffle and computes chi k
//     b1 = b - a, b2 = c - b, b3 = d - c, n1 = b1 x b2, n2 = b2 x b3, chi = atan2(|b2| (b1 . n2), n1 . n2)   (IUPAC sign)
// in float64, every product and sum rounded on its own, so that the cancelling cross products are NumPy's term for term and only
// sqrt and atan2 can differ from a host evaluation.  The class index is class_base + sum_k (bin_k - 1) 3^(n_chi - 1 - k), summed
// across the lanes.  A residue is independent of every other: no atomics, no dependence on the grid, two calls give the same bytes.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>

#include "common.h"
#include "oneshot.h"

// every float64 product and sum below is rounded separately, as NumPy's are
#pragma clang fp contract(off)

namespace {

constexpr int kLanes = 8;                      // lanes per residue: the longest path has 7 atoms (ARG, LYS)
constexpr int kBlock = 256;                    // threads per workgroup
constexpr int kPerBlock = kBlock / kLanes;     // residues per workgroup
constexpr int kTypes = 20, kPath = 7;

// residue types in the codec's order (design_utils.amino_acids.standard_amino_acids: by one-letter code) and the tail of each
// one's path behind N, CA, CB; ALA and GLY have no chi angle
struct Rotamer { const char* res; int n_chi; const char* tail[4]; };
const Rotamer kRotamers[kTypes] = {
    {"ALA", 0, {}},
    {"CYS", 1, {"SG"}},
    {"ASP", 2, {"CG", "OD1"}},
    {"GLU", 3, {"CG", "CD", "OE1"}},
    {"PHE", 2, {"CG", "CD1"}},
    {"GLY", 0, {}},
    {"HIS", 2, {"CG", "ND1"}},
    {"ILE", 2, {"CG1", "CD1"}},
    {"LYS", 4, {"CG", "CD", "CE", "NZ"}},
    {"LEU", 2, {"CG", "CD1"}},
    {"MET", 3, {"CG", "SD", "CE"}},
    {"ASN", 2, {"CG", "OD1"}},
    {"PRO", 2, {"CG", "CD"}},
    {"GLN", 3, {"CG", "CD", "OE1"}},
    {"ARG", 4, {"CG", "CD", "NE", "CZ"}},
    {"SER", 1, {"OG"}},
    {"THR", 1, {"OG1"}},
    {"VAL", 1, {"CG1"}},
    {"TRP", 2, {"CG", "CD1"}},
    {"TYR", 2, {"CG", "CD1"}},
};
const char* const kHead[3] = {"N", "CA", "CB"};

const char* path_name(int type, int p) { return p < 3 ? kHead[p] : kRotamers[type].tail[p - 3]; }

int class_base(int type) {                     // 3^n_chi classes per residue type, types in order
    int base = 0;
    for (int t = 0; t < type; ++t) {
        int n = 1;
        for (int k = 0; k < kRotamers[t].n_chi; ++k) n *= 3;
        base += n;
    }
    return base;
}

uint32_t pack_name(const char* s) {            // four ASCII bytes, left-justified, zero-padded, little-endian
    uint32_t v = 0;
    for (int i = 0; i < 4 && s[i]; ++i) v |= (uint32_t)(unsigned char)s[i] << (8 * i);
    return v;
}

struct DevEntry { int n_chi, base; uint32_t name[kPath]; };
struct DevTable { DevEntry e[kTypes]; };       // 720 bytes, a kernel argument

DevTable device_table() {
    DevTable t;
    std::memset(&t, 0, sizeof t);
    for (int r = 0; r < kTypes; ++r) {
        t.e[r].n_chi = kRotamers[r].n_chi;
        t.e[r].base = class_base(r);
        for (int p = 0; p < kRotamers[r].n_chi + 3 && kRotamers[r].n_chi > 0; ++p) t.e[r].name[p] = pack_name(path_name(r, p));
    }
    return t;
}

__global__ void __launch_bounds__(kBlock) k_tag_rotamers(const double* __restrict__ xyz, const uint32_t* __restrict__ atom_name,
                                                         const long long* __restrict__ res_offsets, const signed char* __restrict__ res_type,
                                                         long long n_res, int flags, const DevTable tab,
                                                         short* __restrict__ cls_out, double* __restrict__ chi_out) {
    const long long r = (long long)blockIdx.x * kPerBlock + threadIdx.x / kLanes;
    const int lane = threadIdx.x % kLanes;
    const bool live = r < n_res;
    const int type = live ? (int)res_type[r] : -1;
    const int ti = type >= 0 ? type : 0;                               // a table row that exists, whatever the residue
    const int n_chi = type >= 0 ? tab.e[ti].n_chi : 0;
    const int n_path = n_chi > 0 ? n_chi + 3 : 0;
    const double nan = __builtin_nan("");
    double px = nan, py = nan, pz = nan;
    bool missing = false;
    if (lane < n_path) {                                               // the first atom of the residue that carries this lane's name
        const uint32_t want = tab.e[ti].name[lane];
        const long long end = res_offsets[r + 1];
        missing = true;
        for (long long a = res_offsets[r]; a < end; ++a)
            if (atom_name[a] == want) {
                px = xyz[3 * (size_t)a];
                py = xyz[3 * (size_t)a + 1];
                pz = xyz[3 * (size_t)a + 2];
                missing = false;
                break;
            }
    }
    // lane k: a = its own atom, b, c, d = the next three of the path (the values lanes >= n_chi receive are not used)
    const double bx = __shfl_down(px, 1, kLanes), by = __shfl_down(py, 1, kLanes), bz = __shfl_down(pz, 1, kLanes);
    const double cx = __shfl_down(px, 2, kLanes), cy = __shfl_down(py, 2, kLanes), cz = __shfl_down(pz, 2, kLanes);
    const double dx = __shfl_down(px, 3, kLanes), dy = __shfl_down(py, 3, kLanes), dz = __shfl_down(pz, 3, kLanes);
    const double b1x = bx - px, b1y = by - py, b1z = bz - pz;
    const double b2x = cx - bx, b2y = cy - by, b2z = cz - bz;
    const double b3x = dx - cx, b3y = dy - cy, b3z = dz - cz;
    const double n1x = b1y * b2z - b1z * b2y, n1y = b1z * b2x - b1x * b2z, n1z = b1x * b2y - b1y * b2x;
    const double n2x = b2y * b3z - b2z * b3y, n2y = b2z * b3x - b2x * b3z, n2z = b2x * b3y - b2y * b3x;
    const double len2 = sqrt((b2x * b2x + b2y * b2y) + b2z * b2z);
    const double sy = len2 * ((b1x * n2x + b1y * n2y) + b1z * n2z);
    const double sx = (n1x * n2x + n1y * n2y) + n1z * n2z;
    const double chi = atan2(sy, sx) * 57.29577951308232;             // 180 / pi: degrees in (-180, 180]
    const bool mine = lane < n_chi;
    const bool bad = missing || (mine && !(fabs(chi) <= 180.0));       // a NaN coordinate ends here; atan2 itself never overflows
    const int bin = (chi >= 0.0 && chi < 120.0) ? 1 : (chi >= -120.0 && chi < 0.0) ? 3 : 2;
    int weight = 1;
    for (int k = lane + 1; k < n_chi; ++k) weight *= 3;               // 3^(n_chi - 1 - lane): the first angle varies slowest
    int sum = mine ? (bin - 1) * weight : 0;
    sum += __shfl_xor(sum, 1, kLanes);
    sum += __shfl_xor(sum, 2, kLanes);                                 // lanes 0..3 hold the sum over lanes 0..3
    const unsigned long long bad_mask = __ballot(bad);
    const int group = (threadIdx.x % warpSize) / kLanes;
    const bool any_bad = ((bad_mask >> (group * kLanes)) & 0xffull) != 0;
    if (!live) return;
    const bool labelled = type >= 0 && !any_bad && !(n_chi == 0 && (flags & 1));
    if (lane == 0) cls_out[r] = labelled ? (short)(tab.e[ti].base + sum) : (short)-1;
    if (chi_out && lane < 4) chi_out[4 * (size_t)r + lane] = (labelled && mine) ? chi : nan;
}

}  // namespace

extern "C" int th_rotamer_table(int res_type, int* n_chi, int* class_base_out, char names[7][4]) {
    if (res_type < 0 || res_type >= kTypes) TH_FAIL(TH_EINVAL, "th_rotamer_table: residue type %d outside 0..%d", res_type, kTypes - 1);
    const Rotamer& rot = kRotamers[res_type];
    if (n_chi) *n_chi = rot.n_chi;
    if (class_base_out) *class_base_out = class_base(res_type);
    if (names) {
        std::memset(names, 0, 7 * 4);
        for (int p = 0; rot.n_chi > 0 && p < rot.n_chi + 3; ++p) std::strncpy(names[p], path_name(res_type, p), 4);
    }
    return TH_OK;
}

extern "C" int th_tag_rotamers(int device, const double* xyz, const uint32_t* atom_name, int64_t total, const int64_t* res_offsets,
                               const int8_t* res_type, int64_t n_res, int flags, int16_t* cls_out, double* chi_out, double* kernel_ms) {
    if (total < 0 || n_res < 0) TH_FAIL(TH_EINVAL, "th_tag_rotamers: negative size (total = %lld, n_res = %lld)", (long long)total, (long long)n_res);
    if (total > INT_MAX || n_res > INT_MAX)
        TH_FAIL(TH_EINVAL, "th_tag_rotamers: %lld atoms / %lld residues in one call (limit 2^31 - 1 each)", (long long)total, (long long)n_res);
    if (kernel_ms) *kernel_ms = 0.0;
    if (n_res == 0) return TH_OK;
    if (!res_offsets || !res_type || !cls_out || (total > 0 && (!xyz || !atom_name)))
        TH_FAIL(TH_EINVAL, "th_tag_rotamers: n_res = %lld needs res_offsets, res_type and cls_out, total = %lld needs xyz and atom_name",
                (long long)n_res, (long long)total);
    if (res_offsets[0] < 0 || res_offsets[n_res] > total)
        TH_FAIL(TH_EINVAL, "th_tag_rotamers: res_offsets run from %lld to %lld, outside 0..total = %lld", (long long)res_offsets[0],
                (long long)res_offsets[n_res], (long long)total);
    for (int64_t r = 0; r < n_res; ++r) {
        if (res_offsets[r + 1] < res_offsets[r])
            TH_FAIL(TH_EINVAL, "th_tag_rotamers: res_offsets[%lld] > res_offsets[%lld]", (long long)r, (long long)r + 1);
        if (res_type[r] < -1 || res_type[r] >= kTypes)
            TH_FAIL(TH_EINVAL, "th_tag_rotamers: res_type[%lld] = %d outside -1..%d", (long long)r, (int)res_type[r], kTypes - 1);
    }

    const size_t n = (size_t)total, nr = (size_t)n_res;
    ThLayout lay;
    const size_t o_xyz = lay.take(n * 3 * sizeof(double)), o_name = lay.take(n * sizeof(uint32_t)), o_offsets = lay.take((nr + 1) * sizeof(int64_t));
    const size_t o_type = lay.take(nr), o_cls = lay.take(nr * sizeof(int16_t)), o_chi = lay.take(chi_out ? nr * 4 * sizeof(double) : 0);
    ThCall call;
    if (int rc = call.open("th_tag_rotamers", device, lay.bytes, kernel_ms ? 2 : 0)) return rc;
    double* d_xyz = call.at<double>(o_xyz);
    uint32_t* d_name = call.at<uint32_t>(o_name);
    long long* d_offsets = call.at<long long>(o_offsets);
    signed char* d_type = call.at<signed char>(o_type);
    short* d_cls = call.at<short>(o_cls);
    double* d_chi = chi_out ? call.at<double>(o_chi) : nullptr;
    hipStream_t st = call.st[0];
    if (n) {
        HIP_TRY(hipMemcpyAsync(d_xyz, xyz, n * 3 * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_name, atom_name, n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipMemcpyAsync(d_offsets, res_offsets, (nr + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_type, res_type, nr, hipMemcpyHostToDevice, st));
    HIP_TRY(call.mark(0));
    hipLaunchKernelGGL(k_tag_rotamers, dim3((unsigned)((nr + kPerBlock - 1) / kPerBlock)), dim3(kBlock), 0, st, d_xyz, d_name, d_offsets, d_type,
                       (long long)n_res, flags, device_table(), d_cls, d_chi);
    HIP_TRY(hipGetLastError());
    HIP_TRY(call.mark(1));
    HIP_TRY(hipMemcpyAsync(cls_out, d_cls, nr * sizeof(int16_t), hipMemcpyDeviceToHost, st));
    if (chi_out) HIP_TRY(hipMemcpyAsync(chi_out, d_chi, nr * 4 * sizeof(double), hipMemcpyDeviceToHost, st));
    return call.finish(kernel_ms);
}
