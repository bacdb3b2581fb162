// th_lddt: the local Distance Difference Test (Mariani et al. 2013) of a BATCH of position-paired coordinate lists (the CA atoms of a
// model against those of its native) — per position the number of neighbours within the inclusion radius in the native and how many
// of those distances the model preserves within each of four thresholds; per pair their totals.  Superposition-free: the measured
// counterpart of the pLDDT that AlphaFold2 writes into the B-factor column, beside th_superpose's RMSD and GDT.
//
//     *** PARITY UNPINNED AGAINST OPENSTRUCTURE ***  Neither OpenStructure nor AlphaFold's lddt.py is available where this project is
//     built.  The rule — written out in include/timed_hip.h — is this project's reading of the published definition in the CA-only
//     form AlphaFold uses: one position per residue, no stereochemistry checks, strict inequalities on both tests; it is neither
//     implementation's code and no test can pin it against OpenStructure.
//
// k_lddt, the hot path: a work item is (pair, tile of 256 positions i); a thread owns one i and keeps its five counts in registers
// while the positions j of its pair stream through LDS in tiles of 256, both lists (six arrays of doubles; every lane of a wave reads
// the same j: a broadcast, no bank conflict).  An invalid position is staged as NaN in BOTH lists and the last tile is padded with
// NaN, so the inner loop has neither a mask nor a bounds test: a NaN is within no radius.  The inclusion test is on the squared
// distance against th_packing_threshold(radius) — the same decision as sqrt(s) < radius for every double — so the two square roots
// and the four comparisons run for included pairs only, under a branch (TH_LDDT_SKIP, below).  The self pair is counted (distance 0,
// difference 0: included and preserved at every threshold, all of which are > 0) and subtracted at the end, as k_contacts does.
// Letting the wavefronts without a position of their own (3 of the 8 that 300 positions occupy) skip the inner loop was measured
// and changed nothing (2.235 against 2.246 ms for 10 000 pairs of 300), so they run it: their NaN include nothing.
// k_lddt_totals: one wavefront per pair sums the rows into 64-bit integers (integer sums: any order gives the same bytes).
// No atomics; nothing depends on the grid, on arrival order or on a pair's place in the batch: two calls give the same bytes.
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

// 1: the body of an included pair sits under `if (s < threshold)`, which hipcc turns into a jump over it when no lane of the
// wavefront includes this j (consecutive i are neighbours along the chain, so lanes tend to agree).  0: both square roots and the
// comparisons are computed for every j and the result is masked.  The integers are the same; profiles/lddt.txt has both rates.
#ifndef TH_LDDT_SKIP
#define TH_LDDT_SKIP 1
#endif

namespace {

constexpr int kTile = 256;                     // positions i per work item = threads per workgroup = positions j per LDS tile
constexpr int kWave = 64;
constexpr int kPerBlock = kTile / kWave;       // pairs per workgroup of k_lddt_totals

// finite3(a) && finite3(b) of device_math.h, kept as one chain of six: written with finite3, hipcc folds each half into selects
// before it inlines, and k_lddt's staging loop comes out as other code in other registers (58 -> 56 VGPRs)
__device__ inline bool finite6(const double* a, const double* b) {
    return __builtin_isfinite(a[0]) && __builtin_isfinite(a[1]) && __builtin_isfinite(a[2]) && __builtin_isfinite(b[0]) &&
           __builtin_isfinite(b[1]) && __builtin_isfinite(b[2]);
}

struct Limits { double t[4]; };

__global__ void __launch_bounds__(kTile) k_lddt(const double* __restrict__ ref_xyz, const double* __restrict__ mob_xyz,
                                                const long long* __restrict__ offsets, const ThTile* __restrict__ items, double threshold,
                                                Limits lim, int* __restrict__ residue_out) {
    __shared__ __attribute__((aligned(16))) double rx[kTile], ry[kTile], rz[kTile], mx[kTile], my[kTile], mz[kTile];
    const int tid = threadIdx.x;
    const ThTile it = items[blockIdx.x];       // positions offsets[range] + tile * kTile ... of that pair
    const long long begin = offsets[it.range], end = offsets[it.range + 1];
    const long long i = begin + (long long)it.tile * kTile + tid;
    const bool live = i < end;
    const double nan = __builtin_nan("");
    double ri[3] = {nan, nan, nan}, mi[3] = {nan, nan, nan};
    if (live) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            ri[a] = ref_xyz[3 * i + a];
            mi[a] = mob_xyz[3 * i + a];
        }
    }
    const bool valid = finite6(ri, mi);        // false for a thread beyond the pair
    if (!valid) ri[0] = ri[1] = ri[2] = mi[0] = mi[1] = mi[2] = nan;
    int n = 0, c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    for (long long j0 = begin; j0 < end; j0 += kTile) {
        const long long j = j0 + tid;
        double rj[3] = {nan, nan, nan}, mj[3] = {nan, nan, nan};
        if (j < end) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                rj[a] = ref_xyz[3 * j + a];
                mj[a] = mob_xyz[3 * j + a];
            }
        }
        const bool ok = finite6(rj, mj);
        __syncthreads();                       // the previous tile is no longer read
        rx[tid] = ok ? rj[0] : nan;
        ry[tid] = ok ? rj[1] : nan;
        rz[tid] = ok ? rj[2] : nan;
        mx[tid] = ok ? mj[0] : nan;
        my[tid] = ok ? mj[1] : nan;
        mz[tid] = ok ? mj[2] : nan;
        __syncthreads();
        const int m = (int)(end - j0 < kTile ? end - j0 : kTile), m2 = (m + 1) & ~1;      // slot m (if m is odd) holds NaN
#pragma unroll 2
        for (int jj = 0; jj < m2; jj += 2) {
            const double2 x = *(const double2*)&rx[jj], y = *(const double2*)&ry[jj], z = *(const double2*)&rz[jj];
            const double xs[2] = {x.x, x.y}, ys[2] = {y.x, y.y}, zs[2] = {z.x, z.y};
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const double dx = xs[u] - ri[0], dy = ys[u] - ri[1], dz = zs[u] - ri[2];
                const double s = (dx * dx + dy * dy) + dz * dz;
#if TH_LDDT_SKIP
                if (s < threshold) {           // false for a NaN
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
                const bool in = s < threshold;
                n += in ? 1 : 0;
                c0 += in && diff < lim.t[0] ? 1 : 0;
                c1 += in && diff < lim.t[1] ? 1 : 0;
                c2 += in && diff < lim.t[2] ? 1 : 0;
                c3 += in && diff < lim.t[3] ? 1 : 0;
#endif
            }
        }
    }
    if (live) {                                // a valid position counted itself in all five; an invalid one counted nothing
        const int self = valid ? 1 : 0;
        int* row = residue_out + 5 * i;
        row[0] = n - self;
        row[1] = c0 - self;
        row[2] = c1 - self;
        row[3] = c2 - self;
        row[4] = c3 - self;
    }
}

__global__ void __launch_bounds__(kTile) k_lddt_totals(const double* __restrict__ ref_xyz, const double* __restrict__ mob_xyz,
                                                       const long long* __restrict__ offsets, long long n_pairs,
                                                       const int* __restrict__ residue, long long* __restrict__ pair_out) {
    const long long pair = (long long)blockIdx.x * kPerBlock + threadIdx.x / kWave;
    if (pair >= n_pairs) return;               // the whole wavefront leaves
    const int lane = threadIdx.x % kWave;
    const long long begin = offsets[pair], end = offsets[pair + 1];
    long long sum[6] = {0, 0, 0, 0, 0, 0};
    for (long long i = begin + lane; i < end; i += kWave) {
        sum[0] += finite6(ref_xyz + 3 * i, mob_xyz + 3 * i) ? 1 : 0;
#pragma unroll
        for (int k = 0; k < 5; ++k) sum[1 + k] += residue[5 * i + k];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) sum[k] = wave_sum(sum[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) pair_out[6 * pair + k] = sum[k];
    }
}

}  // namespace

extern "C" int th_lddt(int device, const double* ref_xyz, const double* mob_xyz, int64_t total, const int64_t* offsets, int64_t n_pairs,
                       double radius, const double* thresholds, int32_t* residue_out, int64_t* pair_out, double* kernel_ms) {
    if (total < 0 || n_pairs < 0) TH_FAIL(TH_EINVAL, "th_lddt: negative size (total = %lld, n_pairs = %lld)", (long long)total, (long long)n_pairs);
    if (total > INT_MAX || n_pairs > INT_MAX)
        TH_FAIL(TH_EINVAL, "th_lddt: %lld positions / %lld pairs in one call (limit 2^31 - 1 each)", (long long)total, (long long)n_pairs);
    if (!std::isfinite(radius) || radius <= 0.0) TH_FAIL(TH_EINVAL, "th_lddt: radius = %g is not a positive finite number", radius);
    if (!thresholds) TH_FAIL(TH_EINVAL, "th_lddt: thresholds is NULL (four doubles)");
    Limits lim;
    for (int k = 0; k < 4; ++k) {
        if (!std::isfinite(thresholds[k]) || thresholds[k] <= 0.0)
            TH_FAIL(TH_EINVAL, "th_lddt: thresholds[%d] = %g is not a positive finite number", k, thresholds[k]);
        lim.t[k] = thresholds[k];
    }
    if (n_pairs == 0) {
        if (total != 0) TH_FAIL(TH_EINVAL, "th_lddt: n_pairs = 0 owns no position, total = %lld", (long long)total);
        if (kernel_ms) *kernel_ms = 0.0;
        return TH_OK;
    }
    if (!offsets || !pair_out || (total > 0 && (!ref_xyz || !mob_xyz || !residue_out)))
        TH_FAIL(TH_EINVAL, "th_lddt: n_pairs = %lld needs offsets and pair_out, total = %lld needs ref_xyz, mob_xyz and residue_out",
                (long long)n_pairs, (long long)total);
    if (int rc = th_check_offsets("th_lddt", "offsets", "total", offsets, n_pairs, total)) return rc;
    std::vector<ThTile> items;
    if (int rc = th_tile_items("th_lddt", "positions", offsets, n_pairs, kTile, items)) return rc;

    const size_t n = (size_t)total, np = (size_t)n_pairs;
    ThLayout lay;
    const size_t o_ref = lay.take(n * 3 * sizeof(double)), o_mob = lay.take(n * 3 * sizeof(double));
    const size_t o_offsets = lay.take((np + 1) * sizeof(int64_t)), o_items = lay.take(items.size() * sizeof(ThTile));
    const size_t o_res = lay.take(n * 5 * sizeof(int32_t)), o_pair = lay.take(np * 6 * sizeof(int64_t));
    ThCall call;
    if (int rc = call.open("th_lddt", device, lay.bytes, kernel_ms ? 2 : 0)) return rc;
    double *d_ref = call.at<double>(o_ref), *d_mob = call.at<double>(o_mob);
    long long *d_offsets = call.at<long long>(o_offsets), *d_pair = call.at<long long>(o_pair);
    ThTile* d_items = call.at<ThTile>(o_items);
    int* d_res = call.at<int>(o_res);
    hipStream_t st = call.st[0];
    if (n) {
        HIP_TRY(hipMemcpyAsync(d_ref, ref_xyz, n * 3 * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_mob, mob_xyz, n * 3 * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(ThTile), hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipMemcpyAsync(d_offsets, offsets, (np + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(call.mark(0));
    if (!items.empty()) {
        hipLaunchKernelGGL(k_lddt, dim3((unsigned)items.size()), dim3(kTile), 0, st, d_ref, d_mob, d_offsets, d_items, th_packing_threshold(radius),
                           lim, d_res);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_lddt_totals, dim3((unsigned)((np + kPerBlock - 1) / kPerBlock)), dim3(kTile), 0, st, d_ref, d_mob, d_offsets,
                       (long long)n_pairs, d_res, d_pair);
    HIP_TRY(hipGetLastError());
    HIP_TRY(call.mark(1));
    if (n) HIP_TRY(hipMemcpyAsync(residue_out, d_res, n * 5 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(pair_out, d_pair, np * 6 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    return call.finish(kernel_ms);
}
