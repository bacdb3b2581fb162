// th_lddt_atoms: the all-atom local Distance Difference Test (Mariani et al. 2013) of a BATCH of atom-paired coordinate lists (the
// heavy atoms of a model against those of its native), with the names of chemically equivalent side-chain atoms (the two ring edges
// of PHE and TYR, the carboxylate oxygens of ASP and GLU, ...) resolved per residue before anything is counted.  The companion of
// th_lddt (CA only), for the side chains that th_build_sidechains and th_pack_sidechains place.
//
//     *** PARITY UNPINNED AGAINST OPENSTRUCTURE ***  OpenStructure is not available where this project is built.  The rule — written
//     out in include/timed_hip.h — is this project's reading of the published definition in float64 with fp contract(off): no
//     stereochemistry checks, no sequence-separation filter, strict inequalities on both tests, a missing model atom costs score.
//     It is not OpenStructure's code and no test can pin it against OpenStructure.
//
// Four kernels on one stream, no atomics, nothing that depends on the grid or on a pair's place in the batch:
//   k_lddt_resolve   a work item is (pair, tile of 256 entries of the host-built list of that pair's partnered atoms); a thread owns
//                    one partnered atom a and keeps its reference coordinates, its own and its partner's model coordinates and the
//                    two sums keep_a, swap_a in registers while the atoms b of its pair stream through LDS as in k_lddt.  A b that
//                    has a partner itself is staged with a NaN reference — it is within no radius — so the has-partner bit costs no
//                    array; b's residue index is the seventh array.
//   k_lddt_decide    one thread per symmetric residue adds the sums of its entries, decides swap_R > keep_R, writes swapped_out and
//                    exchanges the model coordinates of its partner pairs in place (both atoms of a pair lie in its own residue).
//   k_lddt_atoms     k_lddt with the residue index of every staged atom in place of the self subtraction (seven LDS arrays, 13 312
//                    bytes): included is s < threshold AND another residue.  A reference-invalid atom is staged with a NaN
//                    reference, a missing one with NaN model coordinates: included, preserved at no threshold.
//   k_lddt_atoms_totals   one wavefront per pair, 64-bit integer sums.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <new>
#include <vector>

#include "common.h"
#include "device_math.h"
#include "oneshot.h"

// every float64 product and sum below is rounded separately, as the NumPy restatement's are
#pragma clang fp contract(off)

// as TH_LDDT_SKIP of lddt.hip: 1 puts the square roots and comparisons of k_lddt_atoms under the inclusion branch, 0 computes them
// for every j and masks.  The integers are the same; profiles/lddt_atoms.txt has both rates.
#ifndef TH_LDDT_ATOMS_SKIP
#define TH_LDDT_ATOMS_SKIP 1
#endif

namespace {

constexpr int kTile = 256;                     // atoms i (entries, residues) per work item = threads per workgroup = atoms j per LDS tile
constexpr int kWave = 64;
constexpr int kPerBlock = kTile / kWave;       // pairs per workgroup of k_lddt_atoms_totals

struct Limits { double t[4]; };

// x, y, z of atom i, or three NaN when one of them is not finite
__device__ inline void load_or_nan(const double* __restrict__ xyz, long long i, double* out) {
    out[0] = xyz[3 * i];
    out[1] = xyz[3 * i + 1];
    out[2] = xyz[3 * i + 2];
    if (!finite3(out)) out[0] = out[1] = out[2] = __builtin_nan("");
}

__device__ inline int preserved(double d_ref, double ex, double ey, double ez, const Limits& lim) {
    const double diff = fabs(d_ref - sqrt((ex * ex + ey * ey) + ez * ez));
    return (diff < lim.t[0] ? 1 : 0) + (diff < lim.t[1] ? 1 : 0) + (diff < lim.t[2] ? 1 : 0) + (diff < lim.t[3] ? 1 : 0);
}

__global__ void __launch_bounds__(kTile) k_lddt_resolve(const double* __restrict__ ref_xyz, const double* __restrict__ mob_xyz,
                                                        const int* __restrict__ residue, const int* __restrict__ partner,
                                                        const long long* __restrict__ offsets, const int* __restrict__ list,
                                                        const long long* __restrict__ list_offsets, const ThTile* __restrict__ items,
                                                        double threshold, Limits lim, int2* __restrict__ sums) {
    __shared__ __attribute__((aligned(16))) double rx[kTile], ry[kTile], rz[kTile], mx[kTile], my[kTile], mz[kTile];
    __shared__ __attribute__((aligned(8))) int rs[kTile];
    const int tid = threadIdx.x;
    const ThTile it = items[blockIdx.x];       // entries list_offsets[range] + tile * kTile ... of that pair's list
    const long long begin = offsets[it.range], end = offsets[it.range + 1];
    const long long e = list_offsets[it.range] + (long long)it.tile * kTile + tid;
    const bool live = e < list_offsets[it.range + 1];
    const double nan = __builtin_nan("");
    double ra[3] = {nan, nan, nan}, ma[3] = {nan, nan, nan}, mp[3] = {nan, nan, nan};
    int mine = -2;                             // no residue has this index
    if (live) {
        const long long a = list[e];
        load_or_nan(ref_xyz, a, ra);
        load_or_nan(mob_xyz, a, ma);
        load_or_nan(mob_xyz, begin + partner[a], mp);
        mine = residue[a];
    }
    int keep = 0, swap = 0;
    for (long long j0 = begin; j0 < end; j0 += kTile) {
        const long long j = j0 + tid;
        double rj[3] = {nan, nan, nan}, mj[3] = {nan, nan, nan};
        int res = -1;
        if (j < end) {
            load_or_nan(ref_xyz, j, rj);
            load_or_nan(mob_xyz, j, mj);
            res = residue[j];
            if (partner[j] >= 0) rj[0] = rj[1] = rj[2] = nan;      // decisions look only at atoms without a partner
        }
        __syncthreads();                       // the previous tile is no longer read
        rx[tid] = rj[0];
        ry[tid] = rj[1];
        rz[tid] = rj[2];
        mx[tid] = mj[0];
        my[tid] = mj[1];
        mz[tid] = mj[2];
        rs[tid] = res;
        __syncthreads();
        const int m = (int)(end - j0 < kTile ? end - j0 : kTile), m2 = (m + 1) & ~1;      // slot m (if m is odd) holds NaN
#pragma unroll 2
        for (int jj = 0; jj < m2; jj += 2) {
            const double2 x = *(const double2*)&rx[jj], y = *(const double2*)&ry[jj], z = *(const double2*)&rz[jj];
            const int2 r = *(const int2*)&rs[jj];
            const double xs[2] = {x.x, x.y}, ys[2] = {y.x, y.y}, zs[2] = {z.x, z.y};
            const int other[2] = {r.x, r.y};
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const double dx = xs[u] - ra[0], dy = ys[u] - ra[1], dz = zs[u] - ra[2];
                const double s = (dx * dx + dy * dy) + dz * dz;
                if (s < threshold && other[u] != mine) {       // false for a NaN
                    const double d = sqrt(s), bx = mx[jj + u], by = my[jj + u], bz = mz[jj + u];
                    keep += preserved(d, bx - ma[0], by - ma[1], bz - ma[2], lim);
                    swap += preserved(d, bx - mp[0], by - mp[1], bz - mp[2], lim);
                }
            }
        }
    }
    if (live) sums[e] = make_int2(keep, swap);
}

// group g = the partnered atoms of one residue = entries group_start[g] .. group_start[g + 1] of the list
__global__ void __launch_bounds__(kTile) k_lddt_decide(double* __restrict__ mob_xyz, const int* __restrict__ partner,
                                                       const long long* __restrict__ offsets, const int* __restrict__ list,
                                                       const int* __restrict__ group_start, const int* __restrict__ group_pair, long long n_groups,
                                                       const int2* __restrict__ sums, unsigned char* __restrict__ swapped_out,
                                                       unsigned char* __restrict__ group_swapped) {
    const long long g = (long long)blockIdx.x * kTile + threadIdx.x;
    if (g >= n_groups) return;
    const int lo = group_start[g], hi = group_start[g + 1];
    long long keep = 0, swap = 0;
    for (int e = lo; e < hi; ++e) {
        keep += sums[e].x;
        swap += sums[e].y;
    }
    const bool swapped = swap > keep;          // a tie keeps the names
    group_swapped[g] = swapped ? 1 : 0;
    if (!swapped) return;
    const long long begin = offsets[group_pair[g]];
    for (int e = lo; e < hi; ++e) {
        const long long a = list[e], p = begin + partner[a];
        swapped_out[a] = 1;
        if (a < p) {                           // each partner pair once: p is an entry of this group too
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double t = mob_xyz[3 * a + k];
                mob_xyz[3 * a + k] = mob_xyz[3 * p + k];
                mob_xyz[3 * p + k] = t;
            }
        }
    }
}

__global__ void __launch_bounds__(kTile) k_lddt_atoms(const double* __restrict__ ref_xyz, const double* __restrict__ mob_xyz,
                                                      const int* __restrict__ residue, const long long* __restrict__ offsets,
                                                      const ThTile* __restrict__ items, double threshold, Limits lim, int* __restrict__ atom_out) {
    __shared__ __attribute__((aligned(16))) double rx[kTile], ry[kTile], rz[kTile], mx[kTile], my[kTile], mz[kTile];
    __shared__ __attribute__((aligned(8))) int rs[kTile];
    const int tid = threadIdx.x;
    const ThTile it = items[blockIdx.x];       // atoms offsets[range] + tile * kTile ... of that pair
    const long long begin = offsets[it.range], end = offsets[it.range + 1];
    const long long i = begin + (long long)it.tile * kTile + tid;
    const bool live = i < end;
    const double nan = __builtin_nan("");
    double ri[3] = {nan, nan, nan}, mi[3] = {nan, nan, nan};
    int mine = -2;                             // no residue has this index
    if (live) {
        load_or_nan(ref_xyz, i, ri);           // not reference-valid: NaN, within no radius
        load_or_nan(mob_xyz, i, mi);           // missing: NaN, preserved at no threshold
        mine = residue[i];
    }
    int n = 0, c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    for (long long j0 = begin; j0 < end; j0 += kTile) {
        const long long j = j0 + tid;
        double rj[3] = {nan, nan, nan}, mj[3] = {nan, nan, nan};
        int res = -1;
        if (j < end) {
            load_or_nan(ref_xyz, j, rj);
            load_or_nan(mob_xyz, j, mj);
            res = residue[j];
        }
        __syncthreads();                       // the previous tile is no longer read
        rx[tid] = rj[0];
        ry[tid] = rj[1];
        rz[tid] = rj[2];
        mx[tid] = mj[0];
        my[tid] = mj[1];
        mz[tid] = mj[2];
        rs[tid] = res;
        __syncthreads();
        const int m = (int)(end - j0 < kTile ? end - j0 : kTile), m2 = (m + 1) & ~1;      // slot m (if m is odd) holds NaN
#pragma unroll 2
        for (int jj = 0; jj < m2; jj += 2) {
            const double2 x = *(const double2*)&rx[jj], y = *(const double2*)&ry[jj], z = *(const double2*)&rz[jj];
            const int2 r = *(const int2*)&rs[jj];
            const double xs[2] = {x.x, x.y}, ys[2] = {y.x, y.y}, zs[2] = {z.x, z.y};
            const int other[2] = {r.x, r.y};
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const double dx = xs[u] - ri[0], dy = ys[u] - ri[1], dz = zs[u] - ri[2];
                const double s = (dx * dx + dy * dy) + dz * dz;
#if TH_LDDT_ATOMS_SKIP
                if (s < threshold && other[u] != mine) {       // false for a NaN
                    const double ex = mx[jj + u] - mi[0], ey = my[jj + u] - mi[1], ez = mz[jj + u] - mi[2];
                    const double diff = fabs(sqrt(s) - sqrt((ex * ex + ey * ey) + ez * ez));
                    n += 1;
                    c0 += diff < lim.t[0] ? 1 : 0;
                    c1 += diff < lim.t[1] ? 1 : 0;
                    c2 += diff < lim.t[2] ? 1 : 0;
                    c3 += diff < lim.t[3] ? 1 : 0;
                }
#else
                const double ex = mx[jj + u] - mi[0], ey = my[jj + u] - mi[1], ez = mz[jj + u] - mi[2];
                const double diff = fabs(sqrt(s) - sqrt((ex * ex + ey * ey) + ez * ez));
                const bool in = s < threshold && other[u] != mine;
                n += in ? 1 : 0;
                c0 += in && diff < lim.t[0] ? 1 : 0;
                c1 += in && diff < lim.t[1] ? 1 : 0;
                c2 += in && diff < lim.t[2] ? 1 : 0;
                c3 += in && diff < lim.t[3] ? 1 : 0;
#endif
            }
        }
    }
    if (live) {
        int* row = atom_out + 5 * i;
        row[0] = n;
        row[1] = c0;
        row[2] = c1;
        row[3] = c2;
        row[4] = c3;
    }
}

__global__ void __launch_bounds__(kTile) k_lddt_atoms_totals(const double* __restrict__ ref_xyz, const double* __restrict__ mob_xyz,
                                                             const long long* __restrict__ offsets, const long long* __restrict__ group_offsets,
                                                             const unsigned char* __restrict__ group_swapped, long long n_pairs,
                                                             const int* __restrict__ atom, long long* __restrict__ pair_out) {
    const long long pair = (long long)blockIdx.x * kPerBlock + threadIdx.x / kWave;
    if (pair >= n_pairs) return;               // the whole wavefront leaves
    const int lane = threadIdx.x % kWave;
    const long long begin = offsets[pair], end = offsets[pair + 1];
    long long sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (long long i = begin + lane; i < end; i += kWave) {
        const bool in_ref = finite3(ref_xyz + 3 * i);
        sum[0] += in_ref ? 1 : 0;
        sum[1] += in_ref && !finite3(mob_xyz + 3 * i) ? 1 : 0;       // a swap stays inside a residue: the count is that of the model as named
#pragma unroll
        for (int k = 0; k < 5; ++k) sum[2 + k] += atom[5 * i + k];
    }
    for (long long g = group_offsets[pair] + lane; g < group_offsets[pair + 1]; g += kWave) sum[7] += group_swapped[g];
#pragma unroll
    for (int k = 0; k < 8; ++k) sum[k] = wave_sum(sum[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) pair_out[8 * pair + k] = sum[k];
    }
}

}  // namespace

extern "C" int th_lddt_atoms(int device, const double* ref_xyz, const double* mob_xyz, const int32_t* residue, const int32_t* partner,
                             int64_t total, const int64_t* offsets, int64_t n_pairs, double radius, const double* thresholds, unsigned flags,
                             int32_t* atom_out, uint8_t* swapped_out, int64_t* pair_out, double* kernel_ms) {
    if (total < 0 || n_pairs < 0)
        TH_FAIL(TH_EINVAL, "th_lddt_atoms: negative size (total = %lld, n_pairs = %lld)", (long long)total, (long long)n_pairs);
    if (total > INT_MAX || n_pairs > INT_MAX)
        TH_FAIL(TH_EINVAL, "th_lddt_atoms: %lld atoms / %lld pairs in one call (limit 2^31 - 1 each)", (long long)total, (long long)n_pairs);
    if (flags & ~TH_LDDT_NO_SYMMETRY) TH_FAIL(TH_EINVAL, "th_lddt_atoms: unknown flag bits 0x%x", flags & ~TH_LDDT_NO_SYMMETRY);
    if (!std::isfinite(radius) || radius <= 0.0) TH_FAIL(TH_EINVAL, "th_lddt_atoms: radius = %g is not a positive finite number", radius);
    if (!thresholds) TH_FAIL(TH_EINVAL, "th_lddt_atoms: thresholds is NULL (four doubles)");
    Limits lim;
    for (int k = 0; k < 4; ++k) {
        if (!std::isfinite(thresholds[k]) || thresholds[k] <= 0.0)
            TH_FAIL(TH_EINVAL, "th_lddt_atoms: thresholds[%d] = %g is not a positive finite number", k, thresholds[k]);
        lim.t[k] = thresholds[k];
    }
    if (n_pairs == 0) {
        if (total != 0) TH_FAIL(TH_EINVAL, "th_lddt_atoms: n_pairs = 0 owns no atom, total = %lld", (long long)total);
        if (kernel_ms) kernel_ms[0] = kernel_ms[1] = 0.0;
        return TH_OK;
    }
    const bool symmetry = !(flags & TH_LDDT_NO_SYMMETRY);
    if (!offsets || !pair_out || (total > 0 && (!ref_xyz || !mob_xyz || !residue || !atom_out || !swapped_out || (symmetry && !partner))))
        TH_FAIL(TH_EINVAL, "th_lddt_atoms: n_pairs = %lld needs offsets and pair_out, total = %lld needs ref_xyz, mob_xyz, residue, partner "
                           "(unless TH_LDDT_NO_SYMMETRY), atom_out and swapped_out", (long long)n_pairs, (long long)total);
    if (int rc = th_check_offsets("th_lddt_atoms", "offsets", "total", offsets, n_pairs, total)) return rc;
    for (int64_t p = 0; p < n_pairs; ++p) {
        const int64_t begin = offsets[p], end = offsets[p + 1];
        for (int64_t i = begin; i < end; ++i) {
            const int64_t step = (int64_t)residue[i] - (i == begin ? 0 : (int64_t)residue[i - 1]);
            if (i == begin ? step != 0 : (step != 0 && step != 1))
                TH_FAIL(TH_EINVAL, "th_lddt_atoms: residue[%lld] = %d: the residue index starts at 0 in its pair and rises in steps of 0 or 1",
                        (long long)i, residue[i]);
        }
        if (!symmetry) continue;
        for (int64_t i = begin; i < end; ++i) {
            const int64_t q = partner[i];
            if (q == -1) continue;
            if (q < 0 || q >= end - begin) TH_FAIL(TH_EINVAL, "th_lddt_atoms: partner[%lld] = %lld is outside its pair of %lld atoms", (long long)i,
                                                   (long long)q, (long long)(end - begin));
            if (begin + q == i) TH_FAIL(TH_EINVAL, "th_lddt_atoms: partner[%lld] is the atom itself", (long long)i);
            if (residue[begin + q] != residue[i]) TH_FAIL(TH_EINVAL, "th_lddt_atoms: partner[%lld] = %lld lies in another residue", (long long)i, (long long)q);
            if (begin + partner[begin + q] != i)
                TH_FAIL(TH_EINVAL, "th_lddt_atoms: partner[partner[%lld]] = %d is not the atom itself", (long long)i, partner[begin + q]);
        }
    }
    std::vector<ThTile> items, list_items;
    std::vector<int> list, group_start, group_pair;
    std::vector<int64_t> list_offsets, group_offsets;
    if (int rc = th_tile_items("th_lddt_atoms", "atoms", offsets, n_pairs, kTile, items)) return rc;
    try {                                      // the partnered atoms of every pair, in atom order; a residue's are one group
        list_offsets.assign((size_t)n_pairs + 1, 0);
        group_offsets.assign((size_t)n_pairs + 1, 0);
        for (int64_t p = 0; p < n_pairs; ++p) {
            for (int64_t i = offsets[p]; symmetry && i < offsets[p + 1]; ++i) {
                if (partner[i] < 0) continue;
                if (group_pair.empty() || group_pair.back() != (int)p || residue[list.back()] != residue[i]) {
                    group_start.push_back((int)list.size());
                    group_pair.push_back((int)p);
                }
                list.push_back((int)i);
            }
            list_offsets[p + 1] = (int64_t)list.size();
            group_offsets[p + 1] = (int64_t)group_pair.size();
        }
        group_start.push_back((int)list.size());
    } catch (const std::bad_alloc&) {
        TH_FAIL(TH_ENOMEM, "th_lddt_atoms: out of host memory for the list of partnered atoms of %lld atoms", (long long)total);
    }
    if (int rc = th_tile_items("th_lddt_atoms", "partnered atoms", list_offsets.data(), n_pairs, kTile, list_items)) return rc;

    const size_t n = (size_t)total, np = (size_t)n_pairs, nl = list.size(), ng = group_pair.size();
    ThLayout lay;
    const size_t o_ref = lay.take(n * 3 * sizeof(double)), o_mob = lay.take(n * 3 * sizeof(double));
    const size_t o_residue = lay.take(n * sizeof(int32_t)), o_partner = lay.take(n * sizeof(int32_t));
    const size_t o_offsets = lay.take((np + 1) * sizeof(int64_t)), o_items = lay.take(items.size() * sizeof(ThTile));
    const size_t o_list = lay.take(nl * sizeof(int)), o_list_offsets = lay.take((np + 1) * sizeof(int64_t));
    const size_t o_list_items = lay.take(list_items.size() * sizeof(ThTile)), o_sums = lay.take(nl * sizeof(int2));
    const size_t o_group_start = lay.take((ng + 1) * sizeof(int)), o_group_pair = lay.take(ng * sizeof(int));
    const size_t o_group_offsets = lay.take((np + 1) * sizeof(int64_t)), o_group_swapped = lay.take(ng);
    const size_t o_atom = lay.take(n * 5 * sizeof(int32_t)), o_swapped = lay.take(n), o_pair = lay.take(np * 8 * sizeof(int64_t));
    ThCall call;
    if (int rc = call.open("th_lddt_atoms", device, lay.bytes, kernel_ms ? 3 : 0)) return rc;
    double *d_ref = call.at<double>(o_ref), *d_mob = call.at<double>(o_mob);
    int *d_residue = call.at<int>(o_residue), *d_partner = call.at<int>(o_partner), *d_list = call.at<int>(o_list);
    int *d_group_start = call.at<int>(o_group_start), *d_group_pair = call.at<int>(o_group_pair), *d_atom = call.at<int>(o_atom);
    long long *d_offsets = call.at<long long>(o_offsets), *d_list_offsets = call.at<long long>(o_list_offsets);
    long long *d_group_offsets = call.at<long long>(o_group_offsets), *d_pair = call.at<long long>(o_pair);
    ThTile *d_items = call.at<ThTile>(o_items), *d_list_items = call.at<ThTile>(o_list_items);
    int2* d_sums = call.at<int2>(o_sums);
    unsigned char *d_group_swapped = call.at<unsigned char>(o_group_swapped), *d_swapped = call.at<unsigned char>(o_swapped);
    hipStream_t st = call.st[0];
    if (n) {
        HIP_TRY(hipMemcpyAsync(d_ref, ref_xyz, n * 3 * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_mob, mob_xyz, n * 3 * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_residue, residue, n * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(ThTile), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(d_swapped, 0, n, st));
    }
    if (nl) {
        HIP_TRY(hipMemcpyAsync(d_partner, partner, n * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_list, list.data(), nl * sizeof(int), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_list_items, list_items.data(), list_items.size() * sizeof(ThTile), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_group_pair, group_pair.data(), ng * sizeof(int), hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipMemcpyAsync(d_group_start, group_start.data(), (ng + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_offsets, offsets, (np + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_list_offsets, list_offsets.data(), (np + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_group_offsets, group_offsets.data(), (np + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    const double threshold = th_packing_threshold(radius);
    HIP_TRY(call.mark(0));
    if (nl) {
        hipLaunchKernelGGL(k_lddt_resolve, dim3((unsigned)list_items.size()), dim3(kTile), 0, st, d_ref, d_mob, d_residue, d_partner, d_offsets,
                           d_list, d_list_offsets, d_list_items, threshold, lim, d_sums);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_lddt_decide, dim3((unsigned)((ng + kTile - 1) / kTile)), dim3(kTile), 0, st, d_mob, d_partner, d_offsets, d_list,
                           d_group_start, d_group_pair, (long long)ng, d_sums, d_swapped, d_group_swapped);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(call.mark(1));
    if (!items.empty()) {
        hipLaunchKernelGGL(k_lddt_atoms, dim3((unsigned)items.size()), dim3(kTile), 0, st, d_ref, d_mob, d_residue, d_offsets, d_items, threshold, lim,
                           d_atom);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_lddt_atoms_totals, dim3((unsigned)((np + kPerBlock - 1) / kPerBlock)), dim3(kTile), 0, st, d_ref, d_mob, d_offsets,
                       d_group_offsets, d_group_swapped, (long long)n_pairs, d_atom, d_pair);
    HIP_TRY(hipGetLastError());
    HIP_TRY(call.mark(2));
    if (n) {
        HIP_TRY(hipMemcpyAsync(atom_out, d_atom, n * 5 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(swapped_out, d_swapped, n, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipMemcpyAsync(pair_out, d_pair, np * 8 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    return call.finish(kernel_ms, 2);
}
