// th_tmscore: the TM-score (Zhang & Skolnick 2004) of a BATCH of position-paired coordinate lists — the CA atoms of a model against
// those of its native — as the maximum over a fixed schedule of seed superpositions, each refined by a short fixed-point iteration
// of least-squares fits.  The fit is that of th_superpose (horn_fit.h); the search is what th_superpose does not have.
//
//     *** PARITY UNPINNED AGAINST THE TM-score PROGRAM ***  Zhang & Skolnick's TMscore is not available where this project is built.
//     The rule — written out in include/timed_hip.h — is this project's reading of the published definition and search; it is not
//     their code and no test can pin it against their program.
//
// The host counts the valid positions of every pair, compacts them and knows from that count alone how many seeds a pair has.
// k_tm_seeds: one wavefront per (pair, seed), four per 256-thread workgroup.  Lane l owns compacted positions l, l + 64, ... of its
// pair, and the current set of the seed is ONE 64-bit mask per lane in registers (bit b: position l + 64 b) — hence at most
// 64 x 64 = 4096 positions per pair.  "The set did not change" is a wave-wide AND of mask equality.  No per-seed memory, no LDS, no
// barrier: the coordinates are read from global memory (L2) in every pass, the sums are the xor butterflies of horn_fit.h, every lane
// solves the 4 x 4 eigenproblem itself.  A seed leaves 12 bytes: its best score and the number of fits it made.
// k_tm_best: one wavefront per pair scans those scores for the first maximum, sums the fits and RUNS THAT ONE SEED AGAIN — the same
// device function, so the same bits — this time keeping the superposition of its best round, and writes the pair's outputs.
// A pair's arithmetic depends on its own coordinates alone: not on the grid, not on its neighbours; two calls give the same bytes.
// No atomics.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdlib>
#include <new>
#include <vector>

#include "common.h"
#include "horn_fit.h"
#include "oneshot.h"

namespace {

constexpr int kBlock = 256;                       // threads per workgroup
constexpr int kPerBlock = kBlock / kWave;         // wavefronts (seeds, or pairs) per workgroup
constexpr int kWidenings = TH_TM_MAX_WIDENINGS;

struct TmPair {                                   // one per pair, and one more that ends the seed offsets
    long long lo, n;                              // its positions in the caller's lists
    long long clo, m;                             // its valid positions in the compacted lists
    long long slo;                                // its first seed
    long long L;                                  // normalisation length
    double d0;
};

// (W, s) of seed k of a pair with m valid positions: the window lengths m, m div 2, ... >= 4, every start of each
__device__ inline void tm_window(int m, long long k, int& W, int& s) {
    W = m;
    while (k >= m - W + 1) {                      // k < n_seeds(m), so the walk ends before W div 2 < 4
        k -= m - W + 1;
        W /= 2;
    }
    s = (int)k;
}

// One seed: rounds 0 .. `rounds` of fit, score, select.  Returns the best SCORE of the seed (-infinity if none compared greater),
// counts its fits and, with kKeep, leaves the superposition of the first round that reached that score.
template <bool kKeep>
__device__ inline double tm_seed(const double* __restrict__ ref, const double* __restrict__ mob, int m, int W, int s, double d0,
                                 double d_search, double L, int rounds, int lane, int& fits, Fit& best_fit) {
    const int nb = lane < m ? (m - lane + kWave - 1) / kWave : 0;      // positions this lane owns, <= 64
    const int need = m < 3 ? m : 3;
    unsigned long long cur = 0;
    for (int b = 0; b < nb; ++b) {
        const int c = lane + kWave * b;
        if (c >= s && c < s + W) cur |= 1ull << b;
    }
    double best = -__builtin_inf();
    fits = 0;
    for (int r = 0;; ++r) {
        const double count = (double)wave_sum((int)__popcll(cur));
        Fit fit;
        wave_fit(ref, mob, [&](auto visit) {
            for (int b = 0; b < nb; ++b)
                if ((cur >> b) & 1) visit(lane + kWave * b);
        }, count, fit);
        ++fits;
        // the score of this superposition over every valid position, and the next set in the same pass
        double cut = r == 0 ? d_search - 1.0 : d_search + 1.0;
        double sum = 0.0;
        unsigned long long next = 0;
        for (int b = 0; b < nb; ++b) {
            const int c = lane + kWave * b;
            const double d = distance(fit, ref + 3 * c, mob + 3 * c);
            const double q = d / d0;
            sum += 1.0 / (1.0 + q * q);
            if (d < cut) next |= 1ull << b;
        }
        const double score = wave_sum(sum) / L;
        if (score > best) {
            best = score;
            if (kKeep) best_fit = fit;
        }
        if (r >= rounds) break;
        int chosen = wave_sum((int)__popcll(next));
        for (int widened = 0; chosen < need && widened < kWidenings; ++widened) {      // uniform: both are the same in every lane
            cut += 0.5;
            next = 0;
            for (int b = 0; b < nb; ++b) {
                const int c = lane + kWave * b;
                if (distance(fit, ref + 3 * c, mob + 3 * c) < cut) next |= 1ull << b;
            }
            chosen = wave_sum((int)__popcll(next));
        }
        if (chosen < need || __all(next == cur)) break;
        cur = next;
    }
    return best;
}

// kStage exists in the knock-out build only (common.h, TH_TM_STAGE=1): the workgroup first copies the coordinates of its first
// wavefront's pair into LDS and the wavefronts of that pair read them from there.  Measured and not adopted: profiles/tmscore.txt.
template <bool kStage>
__global__ void __launch_bounds__(kBlock) k_tm_seeds(const double* __restrict__ cref, const double* __restrict__ cmob, const TmPair* __restrict__ pairs,
                                                     long long n_pairs, long long n_seeds, int rounds, double* __restrict__ seed_score,
                                                     int* __restrict__ seed_fits, int stage_positions) {
    const long long g = (long long)blockIdx.x * kPerBlock + threadIdx.x / kWave;
    if (!kStage && g >= n_seeds) return;                               // the whole wavefront leaves
    const int lane = threadIdx.x % kWave;
    const long long mine = g < n_seeds ? g : n_seeds - 1;
    long long lo = 0, hi = n_pairs;                                    // the first pair whose seeds end beyond this one
    while (lo < hi) {
        const long long mid = (lo + hi) / 2;
        if (pairs[mid + 1].slo <= mine) lo = mid + 1; else hi = mid;
    }
    const TmPair p = pairs[lo];
    int W, s, fits;
    tm_window((int)p.m, mine - p.slo, W, s);
    const double d_search = fmin(fmax(p.d0, 4.5), 8.0);
    Fit unused;                                                        // tm_seed<false> keeps none
    double best;
#if TH_KNOCKOUTS
    if (kStage) {
        extern __shared__ double staged[];
        __shared__ long long first_pair;
        if (threadIdx.x == 0) first_pair = lo;
        __syncthreads();
        const TmPair f = pairs[first_pair];
        for (int i = threadIdx.x; i < 3 * (int)f.m; i += kBlock) {
            staged[i] = cref[3 * f.clo + i];
            staged[3 * stage_positions + i] = cmob[3 * f.clo + i];
        }
        __syncthreads();
        if (g >= n_seeds) return;
        if (lo == first_pair) {
            best = tm_seed<false>(staged, staged + 3 * stage_positions, (int)p.m, W, s, p.d0, d_search, (double)p.L, rounds, lane, fits, unused);
            if (lane == 0) {
                seed_score[g] = best;
                seed_fits[g] = fits;
            }
            return;
        }
    }
#endif
    best = tm_seed<false>(cref + 3 * p.clo, cmob + 3 * p.clo, (int)p.m, W, s, p.d0, d_search, (double)p.L, rounds, lane, fits, unused);
    if (lane == 0) {
        seed_score[g] = best;
        seed_fits[g] = fits;
    }
}

__global__ void __launch_bounds__(kBlock) k_tm_best(const double* __restrict__ cref, const double* __restrict__ cmob, const TmPair* __restrict__ pairs,
                                                    const int* __restrict__ cidx, long long n_pairs, int rounds, const double* __restrict__ seed_score,
                                                    const int* __restrict__ seed_fits, double* __restrict__ tm_out, long long* __restrict__ count_out,
                                                    double* __restrict__ dist_out, double* __restrict__ transform_out) {
    const long long pair = (long long)blockIdx.x * kPerBlock + threadIdx.x / kWave;
    if (pair >= n_pairs) return;
    const int lane = threadIdx.x % kWave;
    const TmPair p = pairs[pair];
    const long long n_seeds = pairs[pair + 1].slo - p.slo;
    // the first maximum of the seeds' scores: every lane its own seeds in order, then the lanes
    double top = -__builtin_inf();
    long long at = LLONG_MAX, fits_all = 0;
    for (long long k = lane; k < n_seeds; k += kWave) {
        const double v = seed_score[p.slo + k];
        fits_all += seed_fits[p.slo + k];
        if (v > top) {
            top = v;
            at = k;
        }
    }
    for (int mask = kWave / 2; mask >= 1; mask >>= 1) {
        const double v = __shfl_xor(top, mask, kWave);
        const long long k = __shfl_xor(at, mask, kWave);
        if (v > top || (v == top && k < at)) {
            top = v;
            at = k;
        }
    }
    fits_all = wave_sum(fits_all);
    const double nan = __builtin_nan("");
    Fit fit;
    double tm = nan;
    const double* ref = cref + 3 * p.clo;
    const double* mob = cmob + 3 * p.clo;
    const bool found = at != LLONG_MAX;                                // uniform: every lane holds the same (top, at)
    if (found) {
        int W, s, fits;
        tm_window((int)p.m, at, W, s);
        tm = tm_seed<true>(ref, mob, (int)p.m, W, s, p.d0, fmin(fmax(p.d0, 4.5), 8.0), (double)p.L, rounds, lane, fits, fit);
    }
    if (dist_out)
        for (long long i = lane; i < p.n; i += kWave) {
            const int c = cidx[p.lo + i];                              // the compacted index of position i, -1 at an invalid one
            dist_out[p.lo + i] = found && c >= 0 ? distance(fit, ref + 3 * c, mob + 3 * c) : nan;
        }
    if (lane != 0) return;
    tm_out[2 * pair] = tm;
    tm_out[2 * pair + 1] = p.d0;
    long long* count = count_out + 4 * pair;
    count[0] = p.m;
    count[1] = p.L;
    count[2] = n_seeds;
    count[3] = fits_all;
    if (transform_out) store(fit, transform_out + 12 * pair);          // the identity when nothing is valid
}

long long tm_seed_count(long long m) {
    long long seeds = 0;
    for (long long W = m; W >= 1; W /= 2) {
        seeds += m - W + 1;
        if (W / 2 < 4) break;
    }
    return seeds;
}

}  // namespace

extern "C" double th_tm_d0(int64_t L) {
    if (L <= 15) return 0.5;
    const double d0 = 1.24 * std::cbrt((double)(L - 15)) - 1.8;
    return d0 > 0.5 ? d0 : 0.5;
}

extern "C" int th_tmscore(int device, const double* ref_xyz, const double* mob_xyz, int64_t total, const int64_t* offsets, int64_t n_pairs,
                          const int32_t* norm_len, int rounds, double* tm_out, int64_t* count_out, double* dist_out, double* transform_out,
                          double* kernel_ms) {
    if (total < 0 || n_pairs < 0) TH_FAIL(TH_EINVAL, "th_tmscore: negative size (total = %lld, n_pairs = %lld)", (long long)total, (long long)n_pairs);
    if (total > INT_MAX || n_pairs > INT_MAX)
        TH_FAIL(TH_EINVAL, "th_tmscore: %lld positions / %lld pairs in one call (limit 2^31 - 1 each)", (long long)total, (long long)n_pairs);
    if (rounds < 0) TH_FAIL(TH_EINVAL, "th_tmscore: rounds = %d is negative", rounds);
    if (n_pairs == 0) {
        if (total != 0) TH_FAIL(TH_EINVAL, "th_tmscore: n_pairs = 0 owns no position, total = %lld", (long long)total);
        if (kernel_ms) *kernel_ms = 0.0;
        return TH_OK;
    }
    if (!offsets || !tm_out || !count_out || (total > 0 && (!ref_xyz || !mob_xyz)))
        TH_FAIL(TH_EINVAL, "th_tmscore: n_pairs = %lld needs offsets, tm_out and count_out, total = %lld needs ref_xyz and mob_xyz", (long long)n_pairs,
                (long long)total);
    if (int rc = th_check_offsets("th_tmscore", "offsets", "total", offsets, n_pairs, total)) return rc;
    for (int64_t p = 0; p < n_pairs; ++p) {
        const int64_t n = offsets[p + 1] - offsets[p];
        if (n > TH_TM_MAX_POSITIONS)
            TH_FAIL(TH_EINVAL, "th_tmscore: pair %lld has %lld positions (limit TH_TM_MAX_POSITIONS = %d)", (long long)p, (long long)n, TH_TM_MAX_POSITIONS);
        if (norm_len && norm_len[p] < n)
            TH_FAIL(TH_EINVAL, "th_tmscore: norm_len[%lld] = %d is below the pair's %lld positions", (long long)p, (int)norm_len[p], (long long)n);
    }

    // the valid positions of every pair, compacted in index order; a pair's seeds follow from their number
    const size_t n = (size_t)total, np = (size_t)n_pairs;
    std::vector<TmPair> pairs;
    std::vector<int> cidx;
    std::vector<double> cref, cmob;
    long long n_seeds = 0;
    try {
        pairs.resize(np + 1);
        cidx.resize(n);
        cref.reserve(3 * n);
        cmob.reserve(3 * n);
        for (size_t p = 0; p < np; ++p) {
            TmPair& q = pairs[p];
            q.lo = offsets[p];
            q.n = offsets[p + 1] - offsets[p];
            q.clo = (long long)(cref.size() / 3);
            for (long long i = q.lo; i < q.lo + q.n; ++i) {
                const double* r = ref_xyz + 3 * i;
                const double* m = mob_xyz + 3 * i;
                const bool ok = finite3(r) && finite3(m);
                cidx[(size_t)i] = ok ? (int)(cref.size() / 3 - (size_t)q.clo) : -1;
                if (ok) {
                    cref.insert(cref.end(), r, r + 3);
                    cmob.insert(cmob.end(), m, m + 3);
                }
            }
            q.m = (long long)(cref.size() / 3) - q.clo;
            q.slo = n_seeds;
            q.L = norm_len ? norm_len[p] : q.n;
            q.d0 = th_tm_d0(q.L);
            n_seeds += tm_seed_count(q.m);
        }
        pairs[np] = TmPair{total, 0, (long long)(cref.size() / 3), 0, n_seeds, 0, 0.5};
    } catch (const std::bad_alloc&) {
        TH_FAIL(TH_ENOMEM, "th_tmscore: out of host memory for the valid positions of %lld positions", (long long)total);
    }
    if (n_seeds > INT_MAX)
        TH_FAIL(TH_EINVAL, "th_tmscore: %lld seeds in one call (limit 2^31 - 1): submit fewer pairs at once", n_seeds);
    const size_t nc = cref.size() / 3, ns = (size_t)n_seeds;

    ThLayout lay;
    const size_t o_ref = lay.take(nc * 3 * sizeof(double)), o_mob = lay.take(nc * 3 * sizeof(double)), o_pairs = lay.take((np + 1) * sizeof(TmPair));
    const size_t o_cidx = lay.take(n * sizeof(int)), o_score = lay.take(ns * sizeof(double)), o_fits = lay.take(ns * sizeof(int));
    const size_t o_tm = lay.take(np * 2 * sizeof(double)), o_count = lay.take(np * 4 * sizeof(int64_t));
    const size_t o_dist = lay.take(dist_out ? n * sizeof(double) : 0), o_tr = lay.take(transform_out ? np * 12 * sizeof(double) : 0);
    ThCall call;
    if (int rc = call.open("th_tmscore", device, lay.bytes, kernel_ms ? 2 : 0)) return rc;
    double *d_ref = call.at<double>(o_ref), *d_mob = call.at<double>(o_mob), *d_score = call.at<double>(o_score), *d_tm = call.at<double>(o_tm);
    double* d_dist = dist_out && n ? call.at<double>(o_dist) : nullptr;
    double* d_tr = transform_out ? call.at<double>(o_tr) : nullptr;
    TmPair* d_pairs = call.at<TmPair>(o_pairs);
    int *d_cidx = call.at<int>(o_cidx), *d_fits = call.at<int>(o_fits);
    long long* d_count = call.at<long long>(o_count);
    hipStream_t st = call.st[0];
    if (nc) {
        HIP_TRY(hipMemcpyAsync(d_ref, cref.data(), nc * 3 * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_mob, cmob.data(), nc * 3 * sizeof(double), hipMemcpyHostToDevice, st));
    }
    if (n) HIP_TRY(hipMemcpyAsync(d_cidx, cidx.data(), n * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_pairs, pairs.data(), (np + 1) * sizeof(TmPair), hipMemcpyHostToDevice, st));
    HIP_TRY(call.mark(0));
    if (ns) {
        const dim3 grid((unsigned)((ns + kPerBlock - 1) / kPerBlock));
        bool staged = false;
#if TH_KNOCKOUTS
        long long longest = 0;
        for (size_t p = 0; p < np; ++p) longest = pairs[p].m > longest ? pairs[p].m : longest;
        const char* knob = getenv("TH_TM_STAGE");
        staged = knob && atoi(knob) == 1 && longest * 48 <= 64 * 1024;
        if (staged)
            hipLaunchKernelGGL(k_tm_seeds<true>, grid, dim3(kBlock), (size_t)longest * 48, st, d_ref, d_mob, d_pairs, (long long)n_pairs, n_seeds, rounds,
                               d_score, d_fits, (int)longest);
#endif
        if (!staged)
            hipLaunchKernelGGL(k_tm_seeds<false>, grid, dim3(kBlock), 0, st, d_ref, d_mob, d_pairs, (long long)n_pairs, n_seeds, rounds, d_score, d_fits, 0);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_tm_best, dim3((unsigned)((np + kPerBlock - 1) / kPerBlock)), dim3(kBlock), 0, st, d_ref, d_mob, d_pairs, d_cidx,
                       (long long)n_pairs, rounds, d_score, d_fits, d_tm, d_count, d_dist, d_tr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(call.mark(1));
    HIP_TRY(hipMemcpyAsync(tm_out, d_tm, np * 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(count_out, d_count, np * 4 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (d_dist) HIP_TRY(hipMemcpyAsync(dist_out, d_dist, n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (transform_out) HIP_TRY(hipMemcpyAsync(transform_out, d_tr, np * 12 * sizeof(double), hipMemcpyDeviceToHost, st));
    return call.finish(kernel_ms);
}
