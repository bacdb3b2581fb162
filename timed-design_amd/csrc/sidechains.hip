// th_build_sidechains: the inverse of th_tag_rotamers (rotamers.hip) for a BATCH of structures — from N, CA, C, a residue type and
// chi angles per residue to every side-chain heavy atom, then two measures of the result: the deviation from native atoms of the
// same name and the steric clashes of the built atoms.  The reference closes this gap with SCWRL4 (analyse_rotamers.py analyses 2
// and 3, pack_sidechains); here the rotamer CHOICE is the caller's (a predicted class, the native angles) and nothing is searched.
//
//     *** PARITY UNPINNED AGAINST SCWRL4 ***  SCWRL4 is not available where this project is built.  The tree, its values and the
//     rules below are this project's own (sidechain_table.h; written out in include/timed_hip.h) and no test can pin them against
//     SCWRL4 itself.
//
// k_build_sidechains: 16 lanes per residue, 16 residues per workgroup.  Lanes 0..2 hold N, CA, C; lane 3 + j owns side-chain atom j
// of the residue's type (at most 10, TRP).  A loop runs over tree depth (the table's: 6 levels, ARG and TRP); at each level every
// lane fetches its three parents from their lanes by shuffle and the lanes whose atom has that depth place it (sidechain_place.h,
// shared with the packer's candidates):
//     bc = (c - b) / |c - b|,  n = (b - a) x bc, normalised,  m = n x bc,
//     d = c + ((-(L cos t)) bc + ((L sin t) cos p) m) + ((L sin t) sin p) n        t = bond angle, p = dihedral (IUPAC sign)
// in float64, every product and sum rounded on its own; -(L cos t) and L sin t come from the host with the table.  A NaN backbone
// coordinate, a NaN chi angle that the type needs, or N, CA, C on a line (0 / 0 in the normal) reach the atom as NaN and from there
// every atom below it: the residue is then UNBUILT — all atoms NaN, n_built 0 — never a fault.  With native atoms given, the lane
// of a built atom then scans its residue's native atoms for its packed name (the first wins, as in k_tag_rotamers) and lane 0 sums
// the squared deviations in table order.
//
// k_sidechain_clashes, in the style of k_lddt: a work item is (structure, 24 residues); thread t < 240 owns side-chain slot t % 10
// of residue t / 10 and keeps its two counts in registers while the structure's atoms stream through LDS in tiles of 256 slots, 14
// per residue (N, CA, C, O, ten side-chain slots; absent ones are NaN and are within no distance).  The squared distance
// (dx dx + dy dy) + dz dz is compared with th_packing_threshold(clash_distance) — the same decision as sqrt(s) < distance for every
// double — and the pair rules are evaluated under that branch only.  k_clash_totals: one wavefront per structure sums the rows.
// No atomics; a structure's outputs depend on its own residues alone, not on its place in the batch: two calls give the same bytes.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "common.h"
#include "device_math.h"
#include "oneshot.h"
#include "sidechain_place.h"

// every float64 product and sum below is rounded separately, as the NumPy restatement's are
#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
constexpr int kPerBlock = kBlock / kLanes;     // residues per workgroup of k_build_sidechains
constexpr int kTile = 256;                     // slots j per LDS tile of k_sidechain_clashes = its threads
constexpr int kJSlots = 4 + kScMaxAtoms;       // slots per residue on the j side: N, CA, C, O, side chain
constexpr int kTileRes = 24;                   // residues per work item on the i side: 240 of 256 threads own a side-chain slot
constexpr int kWave = 64;

__global__ void __launch_bounds__(kBlock) k_build_sidechains(const double* __restrict__ backbone, int nb, const signed char* __restrict__ res_type,
                                                             const double* __restrict__ chi, long long n_res,
                                                             const double* __restrict__ nat_xyz, const uint32_t* __restrict__ nat_name,
                                                             const long long* __restrict__ nat_offsets, const signed char* __restrict__ nat_type,
                                                             double* __restrict__ out_xyz, int* __restrict__ out_n_built,
                                                             int* __restrict__ out_n_matched, double* __restrict__ out_sum_sq) {
    const long long r = (long long)blockIdx.x * kPerBlock + threadIdx.x / kLanes;
    const int lane = threadIdx.x % kLanes;
    const bool live = r < n_res;
    const int type = live ? (int)res_type[r] : -1;
    const int ti = type >= 0 ? type : 0;                               // a table row that exists, whatever the residue
    const int n_atoms = type >= 0 ? c_tab.n[ti] : 0;
    const int j = lane - 3;
    const bool mine = j >= 0 && j < n_atoms;
    const int jr = mine ? j : 0;
    const DevRow& row = c_tab.row[ti][jr];
    const double nan = __builtin_nan("");
    double px = nan, py = nan, pz = nan;
    if (live && lane < 3) {
        const size_t at = ((size_t)r * nb + lane) * 3;
        px = backbone[at], py = backbone[at + 1], pz = backbone[at + 2];
    }
    sc_place_lanes(row, mine, mine && row.k >= 0 ? chi[4 * (size_t)r + row.k] : 0.0, px, py, pz);
    const bool bad = (lane < 3 || mine) && !finite3(px, py, pz);
    const unsigned long long bad_mask = __ballot(bad);
    const int group = (threadIdx.x % warpSize) / kLanes;
    const bool built = n_atoms > 0 && ((bad_mask >> (group * kLanes)) & 0xffffull) == 0;
    // the deviation from the native: the first native atom of this residue with this lane's name, where the types agree
    double sq = 0.0;
    int hit = 0;
    if (nat_offsets && live && mine && built && (int)nat_type[r] == type) {
        const long long end = nat_offsets[r + 1];
        for (long long a = nat_offsets[r]; a < end; ++a)
            if (nat_name[a] == row.name) {
                const double qx = nat_xyz[3 * (size_t)a], qy = nat_xyz[3 * (size_t)a + 1], qz = nat_xyz[3 * (size_t)a + 2];
                if (finite3(qx, qy, qz)) {
                    const double dx = px - qx, dy = py - qy, dz = pz - qz;
                    sq = (dx * dx + dy * dy) + dz * dz;
                    hit = 1;
                }
                break;
            }
    }
    double sum_sq = 0.0;
    int n_matched = 0;
    for (int a = 0; a < kScMaxAtoms; ++a) {                            // in table order, unmatched atoms skipped: the restatement's sum
        const double s = __shfl(sq, 3 + a, kLanes);
        const int h = __shfl(hit, 3 + a, kLanes);
        if (h) sum_sq = sum_sq + s;
        n_matched += h;
    }
    if (!live) return;
    if (j >= 0 && j < kScMaxAtoms) {
        double* out = out_xyz + ((size_t)r * kScMaxAtoms + j) * 3;
        const bool keep = built && mine;
        out[0] = keep ? px : nan;
        out[1] = keep ? py : nan;
        out[2] = keep ? pz : nan;
    }
    if (lane == 0) {
        out_n_built[r] = built ? n_atoms : 0;
        if (out_n_matched) out_n_matched[r] = n_matched;
        if (out_sum_sq) out_sum_sq[r] = sum_sq;
    }
}

__global__ void __launch_bounds__(kTile) k_sidechain_clashes(const double* __restrict__ backbone, int nb, const double* __restrict__ sc_xyz,
                                                             const signed char* __restrict__ res_type, const int* __restrict__ chain_id,
                                                             const long long* __restrict__ offsets, const ThTile* __restrict__ items,
                                                             double threshold, int* __restrict__ res_count) {
    __shared__ double jx[kTile], jy[kTile], jz[kTile];
    __shared__ int jmeta[kTile], jchain[kTile], cnt_sc[kTile], cnt_bb[kTile];
    const int tid = threadIdx.x;
    const ThTile it = items[blockIdx.x];       // residues offsets[range] + tile * kTileRes ... of that structure
    const long long begin = offsets[it.range], end = offsets[it.range + 1];
    const int len = (int)(end - begin);
    const int ri = it.tile * kTileRes + tid / kScMaxAtoms, slot = tid % kScMaxAtoms;
    const bool live = tid < kTileRes * kScMaxAtoms && ri < len;
    const double nan = __builtin_nan("");
    double pi[3] = {nan, nan, nan};
    int chain_i = 0;
    bool sg_i = false;
    if (live) {
        const size_t r = (size_t)(begin + ri);
        for (int a = 0; a < 3; ++a) pi[a] = sc_xyz[(r * kScMaxAtoms + slot) * 3 + a];
        chain_i = chain_id ? chain_id[r] : 0;
        const int type = res_type[r];
        sg_i = type >= 0 && slot < c_tab.n[type] && c_tab.row[type][slot].name == c_tab.sg;
    }
    int n_sc = 0, n_bb = 0;
    const long long slots = (long long)len * kJSlots;
    for (long long j0 = 0; j0 < slots; j0 += kTile) {
        const long long j = j0 + tid;
        double pj[3] = {nan, nan, nan};
        int meta = 0, chain_j = 0;
        if (j < slots) {
            const int rj = (int)(j / kJSlots), k = (int)(j % kJSlots);
            const size_t r = (size_t)(begin + rj);
            const int type = res_type[r];
            if (k < 4) {
                if (k < nb)
                    for (int a = 0; a < 3; ++a) pj[a] = backbone[(r * nb + k) * 3 + a];
            } else {
                for (int a = 0; a < 3; ++a) pj[a] = sc_xyz[(r * kScMaxAtoms + (k - 4)) * 3 + a];
            }
            const bool sg_j = k >= 4 && type >= 0 && k - 4 < c_tab.n[type] && c_tab.row[type][k - 4].name == c_tab.sg;
            meta = rj * 4 + (k >= 4 ? 1 : 0) + (sg_j ? 2 : 0);
            chain_j = chain_id ? chain_id[r] : 0;
        }
        __syncthreads();                       // the previous tile is no longer read
        jx[tid] = pj[0];
        jy[tid] = pj[1];
        jz[tid] = pj[2];
        jmeta[tid] = meta;
        jchain[tid] = chain_j;
        __syncthreads();
        const int m = (int)(slots - j0 < kTile ? slots - j0 : kTile);
        for (int jj = 0; jj < m; ++jj) {
            const double dx = jx[jj] - pi[0], dy = jy[jj] - pi[1], dz = jz[jj] - pi[2];
            const double s = (dx * dx + dy * dy) + dz * dz;
            if (s < threshold) {               // false for a NaN: an absent atom on either side
                const int mj = jmeta[jj], rj = mj >> 2;
                const bool sc_j = mj & 1, sg_j = mj & 2;
                const bool neighbour = (rj - ri == 1 || ri - rj == 1) && jchain[jj] == chain_i;
                if (rj != ri && !(sg_i && sg_j) && (sc_j || !neighbour)) {
                    n_sc += sc_j ? 1 : 0;
                    n_bb += sc_j ? 0 : 1;
                }
            }
        }
    }
    cnt_sc[tid] = n_sc;
    cnt_bb[tid] = n_bb;
    __syncthreads();
    if (live && slot == 0) {
        int a = 0, b = 0;
        for (int k = 0; k < kScMaxAtoms; ++k) {
            a += cnt_sc[tid + k];
            b += cnt_bb[tid + k];
        }
        res_count[2 * (size_t)(begin + ri)] = a;
        res_count[2 * (size_t)(begin + ri) + 1] = b;
    }
}

// one wavefront per structure: clashes[r] = both counts of the residue; pairs = side chain against backbone once, side chain
// against side chain seen from both ends and halved
__global__ void __launch_bounds__(kTile) k_clash_totals(const long long* __restrict__ offsets, long long n_struct, const int* __restrict__ res_count,
                                                        int* __restrict__ clashes_out, long long* __restrict__ pairs_out) {
    const long long s = (long long)blockIdx.x * (kTile / kWave) + threadIdx.x / kWave;
    if (s >= n_struct) return;                 // the whole wavefront leaves
    const int lane = threadIdx.x % kWave;
    long long both = 0, bb = 0;
    for (long long r = offsets[s] + lane; r < offsets[s + 1]; r += kWave) {
        const int a = res_count[2 * r], b = res_count[2 * r + 1];
        if (clashes_out) clashes_out[r] = a + b;
        both += a;
        bb += b;
    }
    both = wave_sum(both);
    bb = wave_sum(bb);
    if (lane == 0 && pairs_out) pairs_out[s] = bb + both / 2;
}

}  // namespace

extern "C" int th_sidechain_table(int res_type, int* n_atoms, char names[10][4], int8_t parents[10][3], int8_t chi_index[10],
                                  double geometry[10][3], int* n_closure, int8_t closure_atoms[2][2], double closure_length[2]) {
    if (res_type < 0 || res_type >= kScTypes) TH_FAIL(TH_EINVAL, "th_sidechain_table: residue type %d outside 0..%d", res_type, kScTypes - 1);
    const ScType& sc = kSidechains[res_type];
    if (n_atoms) *n_atoms = sc.n;
    if (names) std::memset(names, 0, kScMaxAtoms * 4);
    if (parents) std::memset(parents, 0, kScMaxAtoms * 3);
    if (chi_index) std::memset(chi_index, -1, kScMaxAtoms);
    if (geometry) std::memset(geometry, 0, kScMaxAtoms * 3 * sizeof(double));
    for (int j = 0; j < sc.n; ++j) {
        const ScRow& row = sc.row[j];
        if (names) std::strncpy(names[j], row.name, 4);
        if (parents) parents[j][0] = row.a, parents[j][1] = row.b, parents[j][2] = row.c;
        if (chi_index) chi_index[j] = row.k;
        if (geometry) geometry[j][0] = row.length, geometry[j][1] = row.angle, geometry[j][2] = row.offset;
    }
    if (n_closure) *n_closure = sc.n_closure;
    for (int q = 0; q < kScMaxClosure; ++q) {
        const bool have = q < sc.n_closure;
        if (closure_atoms) closure_atoms[q][0] = have ? sc.closure[q].a : -1, closure_atoms[q][1] = have ? sc.closure[q].b : -1;
        if (closure_length) closure_length[q] = have ? sc.closure[q].length : 0.0;
    }
    return TH_OK;
}

extern "C" int th_build_sidechains(int device, const double* backbone, const int8_t* res_type, const double* chi, const int32_t* chain_id,
                                   const int64_t* struct_offsets, int64_t n_struct, int64_t n_res, const double* native_xyz,
                                   const uint32_t* native_name, int64_t native_total, const int64_t* native_res_offsets,
                                   const int8_t* native_type, double clash_distance, int flags, double* out_xyz, int32_t* out_n_built,
                                   int32_t* out_n_matched, double* out_sum_sq, int32_t* out_clashes, int64_t* out_struct_pairs,
                                   double* kernel_ms) {
    if (n_struct < 0 || n_res < 0 || native_total < 0)
        TH_FAIL(TH_EINVAL, "th_build_sidechains: negative size (n_struct = %lld, n_res = %lld, native_total = %lld)", (long long)n_struct,
                (long long)n_res, (long long)native_total);
    if (n_res > TH_SC_MAX_RESIDUES || n_struct > INT_MAX || native_total > INT_MAX)
        TH_FAIL(TH_EINVAL, "th_build_sidechains: %lld residues / %lld structures / %lld native atoms in one call (limits %d, 2^31 - 1, 2^31 - 1)",
                (long long)n_res, (long long)n_struct, (long long)native_total, TH_SC_MAX_RESIDUES);
    if (flags & ~TH_SC_BACKBONE_O) TH_FAIL(TH_EINVAL, "th_build_sidechains: flags = %d has bits beyond TH_SC_BACKBONE_O", flags);
    const bool want_clashes = out_clashes || out_struct_pairs;
    if (want_clashes && (!std::isfinite(clash_distance) || clash_distance <= 0.0))
        TH_FAIL(TH_EINVAL, "th_build_sidechains: clash_distance = %g is not a positive finite number", clash_distance);
    const bool native = native_res_offsets != nullptr;
    if (!native && (native_xyz || native_name || native_type || native_total > 0 || out_n_matched || out_sum_sq))
        TH_FAIL(TH_EINVAL, "th_build_sidechains: native arrays or outputs without native_res_offsets");
    if (kernel_ms) *kernel_ms = 0.0;
    if (n_struct == 0 && n_res != 0) TH_FAIL(TH_EINVAL, "th_build_sidechains: n_struct = 0 owns no residue, n_res = %lld", (long long)n_res);
    if (n_struct == 0) return TH_OK;
    if (!struct_offsets) TH_FAIL(TH_EINVAL, "th_build_sidechains: n_struct = %lld needs struct_offsets", (long long)n_struct);
    if (int rc = th_check_offsets("th_build_sidechains", "struct_offsets", "n_res", struct_offsets, n_struct, n_res)) return rc;
    if (n_res > 0 && (!backbone || !res_type || !chi || !out_xyz || !out_n_built))
        TH_FAIL(TH_EINVAL, "th_build_sidechains: n_res = %lld needs backbone, res_type, chi, out_xyz and out_n_built", (long long)n_res);
    if (native && n_res > 0) {
        if (!native_type || !out_n_matched || !out_sum_sq || (native_total > 0 && (!native_xyz || !native_name)))
            TH_FAIL(TH_EINVAL, "th_build_sidechains: a native needs native_type, out_n_matched and out_sum_sq, native_total = %lld needs native_xyz and native_name",
                    (long long)native_total);
        if (native_res_offsets[0] < 0 || native_res_offsets[n_res] > native_total)
            TH_FAIL(TH_EINVAL, "th_build_sidechains: native_res_offsets run from %lld to %lld, outside 0..native_total = %lld",
                    (long long)native_res_offsets[0], (long long)native_res_offsets[n_res], (long long)native_total);
    }
    for (int64_t r = 0; r < n_res; ++r) {
        if (res_type[r] < -1 || res_type[r] >= kScTypes)
            TH_FAIL(TH_EINVAL, "th_build_sidechains: res_type[%lld] = %d outside -1..%d", (long long)r, (int)res_type[r], kScTypes - 1);
        if (native) {
            if (native_res_offsets[r + 1] < native_res_offsets[r])
                TH_FAIL(TH_EINVAL, "th_build_sidechains: native_res_offsets[%lld] > native_res_offsets[%lld]", (long long)r, (long long)r + 1);
            if (native_type[r] < -1 || native_type[r] >= kScTypes)
                TH_FAIL(TH_EINVAL, "th_build_sidechains: native_type[%lld] = %d outside -1..%d", (long long)r, (int)native_type[r], kScTypes - 1);
        }
    }
    if (n_res == 0) {
        if (out_struct_pairs) std::memset(out_struct_pairs, 0, (size_t)n_struct * sizeof(int64_t));
        return TH_OK;
    }
    std::vector<ThTile> items;
    if (want_clashes)
        if (int rc = th_tile_items("th_build_sidechains", "residues", struct_offsets, n_struct, kTileRes, items)) return rc;

    const int nb = (flags & TH_SC_BACKBONE_O) ? 4 : 3;
    const size_t nr = (size_t)n_res, ns = (size_t)n_struct, nn = native ? (size_t)native_total : 0;
    ThLayout lay;
    const size_t o_bb = lay.take(nr * nb * 3 * sizeof(double)), o_type = lay.take(nr), o_chi = lay.take(nr * 4 * sizeof(double));
    const size_t o_chain = lay.take(chain_id && want_clashes ? nr * sizeof(int32_t) : 0), o_soff = lay.take((ns + 1) * sizeof(int64_t));
    const size_t o_nxyz = lay.take(nn * 3 * sizeof(double)), o_nname = lay.take(nn * sizeof(uint32_t));
    const size_t o_noff = lay.take(native ? (nr + 1) * sizeof(int64_t) : 0), o_ntype = lay.take(native ? nr : 0);
    const size_t o_xyz = lay.take(nr * kScMaxAtoms * 3 * sizeof(double)), o_built = lay.take(nr * sizeof(int32_t));
    const size_t o_matched = lay.take(native ? nr * sizeof(int32_t) : 0), o_sq = lay.take(native ? nr * sizeof(double) : 0);
    const size_t o_items = lay.take(items.size() * sizeof(ThTile)), o_count = lay.take(want_clashes ? nr * 2 * sizeof(int32_t) : 0);
    const size_t o_clashes = lay.take(want_clashes ? nr * sizeof(int32_t) : 0), o_pairs = lay.take(want_clashes ? ns * sizeof(int64_t) : 0);
    ThCall call;
    if (int rc = call.open("th_build_sidechains", device, lay.bytes, kernel_ms ? 2 : 0)) return rc;
    double *d_bb = call.at<double>(o_bb), *d_chi = call.at<double>(o_chi), *d_nxyz = call.at<double>(o_nxyz), *d_xyz = call.at<double>(o_xyz);
    signed char* d_type = call.at<signed char>(o_type);
    int* d_chain = chain_id && want_clashes ? call.at<int>(o_chain) : nullptr;
    long long *d_soff = call.at<long long>(o_soff), *d_pairs = call.at<long long>(o_pairs);
    uint32_t* d_nname = call.at<uint32_t>(o_nname);
    long long* d_noff = native ? call.at<long long>(o_noff) : nullptr;
    signed char* d_ntype = native ? call.at<signed char>(o_ntype) : nullptr;
    int *d_built = call.at<int>(o_built), *d_count = call.at<int>(o_count), *d_clashes = call.at<int>(o_clashes);
    int* d_matched = native ? call.at<int>(o_matched) : nullptr;
    double* d_sq = native ? call.at<double>(o_sq) : nullptr;
    ThTile* d_items = call.at<ThTile>(o_items);
    hipStream_t st = call.st[0];
    const DevTable& tab = host_table();
    HIP_TRY(hipMemcpyToSymbolAsync(HIP_SYMBOL(c_tab), &tab, sizeof tab, 0, hipMemcpyHostToDevice, st));       // the same bytes every call
    HIP_TRY(hipMemcpyAsync(d_bb, backbone, nr * nb * 3 * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_type, res_type, nr, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_chi, chi, nr * 4 * sizeof(double), hipMemcpyHostToDevice, st));
    if (d_chain) HIP_TRY(hipMemcpyAsync(d_chain, chain_id, nr * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_soff, struct_offsets, (ns + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    if (native) {
        if (nn) {
            HIP_TRY(hipMemcpyAsync(d_nxyz, native_xyz, nn * 3 * sizeof(double), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(d_nname, native_name, nn * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        }
        HIP_TRY(hipMemcpyAsync(d_noff, native_res_offsets, (nr + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_ntype, native_type, nr, hipMemcpyHostToDevice, st));
    }
    if (!items.empty()) HIP_TRY(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(ThTile), hipMemcpyHostToDevice, st));
    HIP_TRY(call.mark(0));
    hipLaunchKernelGGL(k_build_sidechains, dim3((unsigned)((nr + kPerBlock - 1) / kPerBlock)), dim3(kBlock), 0, st, d_bb, nb, d_type, d_chi,
                       (long long)n_res, d_nxyz, d_nname, d_noff, d_ntype, d_xyz, d_built, d_matched, d_sq);
    HIP_TRY(hipGetLastError());
    if (want_clashes) {
        hipLaunchKernelGGL(k_sidechain_clashes, dim3((unsigned)items.size()), dim3(kTile), 0, st, d_bb, nb, d_xyz, d_type, d_chain, d_soff, d_items,
                           th_packing_threshold(clash_distance), d_count);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_clash_totals, dim3((unsigned)((ns + kTile / kWave - 1) / (kTile / kWave))), dim3(kTile), 0, st, d_soff, (long long)n_struct,
                           d_count, d_clashes, d_pairs);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(call.mark(1));
    HIP_TRY(hipMemcpyAsync(out_xyz, d_xyz, nr * kScMaxAtoms * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out_n_built, d_built, nr * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (native) {
        HIP_TRY(hipMemcpyAsync(out_n_matched, d_matched, nr * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_sum_sq, d_sq, nr * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    if (out_clashes) HIP_TRY(hipMemcpyAsync(out_clashes, d_clashes, nr * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (out_struct_pairs) HIP_TRY(hipMemcpyAsync(out_struct_pairs, d_pairs, ns * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    return call.finish(kernel_ms);
}
