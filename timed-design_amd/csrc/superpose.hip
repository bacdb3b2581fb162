// th_superpose: least-squares superposition of a BATCH of position-paired coordinate lists (the CA atoms of a model on those of its
// native), with outlier-rejection refinement — RMSD, the counts behind a GDT and the per-position deviation.  The reference gets
// these one pair at a time from PyMOL's cmd.align (scripts/analyse_af2.py calculate_RMSD_and_gdt).
//
//     *** PARITY UNPINNED AGAINST PYMOL ***  PyMOL is not available where this project is built.  The rule — written out in
//     include/timed_hip.h — is this project's reading of the documented behaviour of cmd.align (cycles 5, cutoff 2.0) on atoms that
//     are already paired; it is not PyMOL's code and no test can pin it against PyMOL.
//
// k_superpose: one wavefront per pair, four pairs per 256-thread workgroup, the whole batch and every refinement cycle in one launch.
// Lane l owns positions l, l + 64, ... of its pair; the kept byte and the distance of a position are written to global memory by the
// lane that owns it and read back by that lane only, so a cycle needs no barrier and no LDS.  The 3 + 3 + 9 float64 sums of a fit
// and the sums of squared distances are reduced by an xor butterfly of shuffles: a + b is b + a, so every lane ends with the same
// bits, and every lane then solves the 4 x 4 eigenproblem of Horn's matrix itself (cyclic Jacobi, at most kSweeps sweeps) — nothing
// is broadcast.  A pair's arithmetic depends on its own coordinates and its lane layout alone: not on the grid, not on its
// neighbours, and two calls give the same bytes.  No atomics.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#include "common.h"
#include "horn_fit.h"
#include "oneshot.h"

namespace {

constexpr int kBlock = 256;                       // threads per workgroup
constexpr int kPerBlock = kBlock / kWave;         // pairs per workgroup

__global__ void __launch_bounds__(kBlock) k_superpose(const double* __restrict__ ref_xyz, const double* __restrict__ mob_xyz,
                                                      const long long* __restrict__ offsets, long long n_pairs, int cycles, double cutoff,
                                                      double* dist_out, unsigned char* kept_out, double* __restrict__ rmsd_out,
                                                      int* __restrict__ count_out, double* __restrict__ transform_out) {
    const long long pair = (long long)blockIdx.x * kPerBlock + threadIdx.x / kWave;
    if (pair >= n_pairs) return;                                       // the whole wavefront leaves: nothing below is a workgroup barrier
    const int lane = threadIdx.x % kWave;
    const long long lo = offsets[pair];
    const long long n = offsets[pair + 1] - lo;
    const double* ref = ref_xyz + 3 * lo;
    const double* mob = mob_xyz + 3 * lo;
    double* dist = dist_out + lo;
    unsigned char* kept = kept_out + lo;
    const double nan = __builtin_nan("");

    // cycle 0 keeps every valid position
    int n_valid = 0;
    for (long long i = lane; i < n; i += kWave) {
        const bool ok = finite3(ref[3 * i], ref[3 * i + 1], ref[3 * i + 2]) && finite3(mob[3 * i], mob[3 * i + 1], mob[3 * i + 2]);
        kept[i] = ok ? 1 : 0;
        dist[i] = nan;
        n_valid += ok ? 1 : 0;
    }
    n_valid = wave_sum(n_valid);

    int n_kept = n_valid, cycles_run = 0;
    double fit_all = nan, rms_kept = nan, sq_all = 0.0;
    Fit fit;
    while (n_valid > 0) {
        // the fit of the kept set
        wave_fit(ref, mob, [&](auto visit) {
            for (long long i = lane; i < n; i += kWave)
                if (kept[i]) visit(i);
        }, (double)n_kept, fit);
        // distances of every valid position under this fit
        double sq_kept = 0.0;
        sq_all = 0.0;
        for (long long i = lane; i < n; i += kWave) {
            const double m[3] = {mob[3 * i], mob[3 * i + 1], mob[3 * i + 2]}, r[3] = {ref[3 * i], ref[3 * i + 1], ref[3 * i + 2]};
            if (!(finite3(m[0], m[1], m[2]) && finite3(r[0], r[1], r[2]))) continue;   // all six loads are issued before the first test
            const double d = distance(fit, r, m);
            dist[i] = d;
            sq_all += d * d;
            if (kept[i]) sq_kept += d * d;
        }
        sq_all = wave_sum(sq_all);
        rms_kept = sqrt(wave_sum(sq_kept) / (double)n_kept);
        if (cycles_run == 0) fit_all = rms_kept;
        if (cycles_run >= cycles || n_valid < 3) break;
        // refinement: drop the kept positions beyond cutoff * rms, unless none is or fewer than 3 would remain
        const double limit = cutoff * rms_kept;
        int drop = 0;
        for (long long i = lane; i < n; i += kWave)
            if (kept[i] && dist[i] > limit) ++drop;
        drop = wave_sum(drop);
        if (drop == 0 || n_kept - drop < 3) break;
        for (long long i = lane; i < n; i += kWave)
            if (kept[i] && dist[i] > limit) kept[i] = 0;
        n_kept -= drop;
        ++cycles_run;
    }

    int within[4] = {0, 0, 0, 0};
    for (long long i = lane; i < n; i += kWave) {
        const double d = dist[i];                                      // NaN (an invalid position) is within nothing
        within[0] += d <= 1.0 ? 1 : 0;
        within[1] += d <= 2.0 ? 1 : 0;
        within[2] += d <= 4.0 ? 1 : 0;
        within[3] += d <= 8.0 ? 1 : 0;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) within[k] = wave_sum(within[k]);
    if (lane != 0) return;
    rmsd_out[3 * pair] = rms_kept;
    rmsd_out[3 * pair + 1] = n_valid > 0 ? sqrt(sq_all / (double)n_valid) : nan;
    rmsd_out[3 * pair + 2] = fit_all;
    int* count = count_out + 7 * pair;
    count[0] = n_valid;
    count[1] = n_kept;
    count[2] = cycles_run;
#pragma unroll
    for (int k = 0; k < 4; ++k) count[3 + k] = within[k];
    if (transform_out) store(fit, transform_out + 12 * pair);          // the identity when nothing is valid
}

}  // namespace

extern "C" int th_superpose(int device, const double* ref_xyz, const double* mob_xyz, int64_t total, const int64_t* offsets, int64_t n_pairs,
                            int cycles, double cutoff, double* dist_out, uint8_t* kept_out, double* rmsd_out, int32_t* count_out,
                            double* transform_out, double* kernel_ms) {
    if (total < 0 || n_pairs < 0) TH_FAIL(TH_EINVAL, "th_superpose: negative size (total = %lld, n_pairs = %lld)", (long long)total, (long long)n_pairs);
    if (total > INT_MAX || n_pairs > INT_MAX)
        TH_FAIL(TH_EINVAL, "th_superpose: %lld positions / %lld pairs in one call (limit 2^31 - 1 each)", (long long)total, (long long)n_pairs);
    if (cycles < 0) TH_FAIL(TH_EINVAL, "th_superpose: cycles = %d is negative", cycles);
    if (!std::isfinite(cutoff) || cutoff <= 0.0) TH_FAIL(TH_EINVAL, "th_superpose: cutoff = %g is not a positive finite number", cutoff);
    if (n_pairs == 0) {
        if (total != 0) TH_FAIL(TH_EINVAL, "th_superpose: n_pairs = 0 owns no position, total = %lld", (long long)total);
        if (kernel_ms) *kernel_ms = 0.0;
        return TH_OK;
    }
    if (!offsets || !rmsd_out || !count_out || (total > 0 && (!ref_xyz || !mob_xyz || !dist_out || !kept_out)))
        TH_FAIL(TH_EINVAL, "th_superpose: n_pairs = %lld needs offsets, rmsd_out and count_out, total = %lld needs ref_xyz, mob_xyz, dist_out and kept_out",
                (long long)n_pairs, (long long)total);
    if (int rc = th_check_offsets("th_superpose", "offsets", "total", offsets, n_pairs, total)) return rc;

    const size_t n = (size_t)total, np = (size_t)n_pairs;
    ThLayout lay;
    const size_t o_ref = lay.take(n * 3 * sizeof(double)), o_mob = lay.take(n * 3 * sizeof(double)), o_offsets = lay.take((np + 1) * sizeof(int64_t));
    const size_t o_dist = lay.take(n * sizeof(double)), o_kept = lay.take(n), o_rmsd = lay.take(np * 3 * sizeof(double));
    const size_t o_count = lay.take(np * 7 * sizeof(int32_t)), o_tr = lay.take(transform_out ? np * 12 * sizeof(double) : 0);
    ThCall call;
    if (int rc = call.open("th_superpose", device, lay.bytes, kernel_ms ? 2 : 0)) return rc;
    double *d_ref = call.at<double>(o_ref), *d_mob = call.at<double>(o_mob), *d_dist = call.at<double>(o_dist), *d_rmsd = call.at<double>(o_rmsd);
    double* d_tr = transform_out ? call.at<double>(o_tr) : nullptr;
    long long* d_offsets = call.at<long long>(o_offsets);
    unsigned char* d_kept = call.at<unsigned char>(o_kept);
    int* d_count = call.at<int>(o_count);
    hipStream_t st = call.st[0];
    if (n) {
        HIP_TRY(hipMemcpyAsync(d_ref, ref_xyz, n * 3 * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_mob, mob_xyz, n * 3 * sizeof(double), hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipMemcpyAsync(d_offsets, offsets, (np + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(call.mark(0));
    hipLaunchKernelGGL(k_superpose, dim3((unsigned)((np + kPerBlock - 1) / kPerBlock)), dim3(kBlock), 0, st, d_ref, d_mob, d_offsets,
                       (long long)n_pairs, cycles, cutoff, d_dist, d_kept, d_rmsd, d_count, d_tr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(call.mark(1));
    if (n) {
        HIP_TRY(hipMemcpyAsync(dist_out, d_dist, n * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(kept_out, d_kept, n, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipMemcpyAsync(rmsd_out, d_rmsd, np * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(count_out, d_count, np * 7 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (transform_out) HIP_TRY(hipMemcpyAsync(transform_out, d_tr, np * 12 * sizeof(double), hipMemcpyDeviceToHost, st));
    return call.finish(kernel_ms);
}
