// th_cealign: sequence-independent structural alignment (CE, Shindyalov & Bourne 1998) of a BATCH of (reference, model) coordinate
// lists of INDEPENDENT length — what the reference gets one pair at a time from PyMOL's cmd.cealign on the CA atoms
// (scripts/analyse_all_properties.py, scripts/analyse_cherrypicked_samples_af2.py).  The alignment is a pairing: th_superpose,
// th_lddt and th_tmscore then score it unchanged.
//
//     *** PARITY UNPINNED AGAINST PYMOL ***  PyMOL is not available where this project is built.  The rule — written out in
//     include/timed_hip.h — is this project's reading of the published CE algorithm with cealign's documented defaults (window 8,
//     d0 3.0, d1 4.0, gap_max 30, the best 20 paths re-scored by RMSD); it is not PyMOL's code and no test can pin it against PyMOL.
//
// The host compacts each list to its valid positions.  Four kernels, all float64, no fused multiply-add:
// k_ce_windows     one thread per window start of every structure: its 21 intra-window distances, so that S is an L1 distance of rows.
// k_ce_similarity  a 16 x 16 tile of (a, b) per workgroup, the 16 + 16 rows staged in LDS; each thread adds its 21 terms in rule order.
// k_ce_paths       one wavefront per (a0, b0), four per workgroup; a wave whose S is not below d0 leaves at once.  Lane g owns gap
//                  candidate g: it adds D(path[k], candidate) over the path by itself, in path order, so the order of addition is that
//                  of the rule.  The path lives in registers — AFP k in lane k mod 64, register k div 64, (a << 16) | b — and is read
//                  with a shuffle from a uniform lane; the step is a wave argmin on (c, g).  The coordinates are read from global
//                  memory (L2), as th_tmscore reads them.  A start leaves 12 bytes: its length and its score.
// k_ce_best        one wavefront (one workgroup) per pair: counts the starts, takes the first TH_CE_KEEP in the order (length
//                  descending, score ascending, start index ascending) by that many scans — every lane its own records in index order,
//                  then the lanes in a fixed tree —, traces each again with the same device function (the same bits), fits it with
//                  horn_fit.h — the sums of the fit in path order, one after the other, in every lane alike — and writes the outputs of the
//                  candidate of smallest RMSD.
// A pair's arithmetic depends on its own coordinates alone: not on the grid, not on its neighbours; two calls give the same bytes.
// No atomics.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <new>
#include <vector>

#include "common.h"
#include "horn_fit.h"
#include "oneshot.h"

// every float64 product, sum and quotient below is rounded on its own, as the NumPy restatement's are
#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;                       // threads per workgroup of k_ce_windows, k_ce_similarity and k_ce_paths
constexpr int kPerBlock = kBlock / kWave;         // starts per workgroup of k_ce_paths
constexpr int kW = TH_CE_WINDOW;
constexpr int kTerms = 21;                        // pairs (p, q), q >= p + 2, inside a window of 8
constexpr int kTile = 16;                         // k_ce_similarity: window starts per side and workgroup
constexpr int kMaxAfps = TH_CE_MAX_POSITIONS / kW;                     // 256: every AFP advances both sides by 8 at least
constexpr int kPathRegs = kMaxAfps / kWave;       // 4

struct CePair {                                   // one per pair, and one more that ends the offsets
    long long alo, na, blo, nb;                   // its positions in the caller's two lists
    long long calo, ma, cblo, mb;                 // its valid positions in the compacted lists
    long long ralo, rblo;                         // its first window start of either side (ma - 7 and mb - 7 of them, or none)
    long long wlo;                                // its first (a, b): (ma - 7)(mb - 7) of them, a-major
    long long tlo;                                // its first tile of k_ce_similarity
};

template <long long CePair::*kField>
__device__ inline long long ce_find(const CePair* __restrict__ pairs, long long n_pairs, long long x) {
    long long lo = 0, hi = n_pairs;               // the first pair whose range ends beyond x
    while (lo < hi) {
        const long long mid = (lo + hi) / 2;
        if (pairs[mid + 1].*kField <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ inline double ce_dist(const double* __restrict__ xyz, int i, int j) {
    const double dx = xyz[3 * i] - xyz[3 * j], dy = xyz[3 * i + 1] - xyz[3 * j + 1], dz = xyz[3 * i + 2] - xyz[3 * j + 2];
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

__global__ void __launch_bounds__(kBlock) k_ce_windows(const double* __restrict__ ca, const double* __restrict__ cb, const CePair* __restrict__ pairs,
                                                       long long n_pairs, long long rows_a, long long rows_b, double* __restrict__ wa,
                                                       double* __restrict__ wb) {
    long long x = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (x >= rows_a + rows_b) return;
    const bool model = x >= rows_a;
    if (model) x -= rows_a;
    const long long p = model ? ce_find<&CePair::rblo>(pairs, n_pairs, x) : ce_find<&CePair::ralo>(pairs, n_pairs, x);
    const CePair q = pairs[p];
    const double* xyz = model ? cb + 3 * q.cblo : ca + 3 * q.calo;
    const int a = (int)(x - (model ? q.rblo : q.ralo));
    double* row = (model ? wb : wa) + kTerms * x;
    int t = 0;
    for (int i = 0; i < kW; ++i)
        for (int j = i + 2; j < kW; ++j) row[t++] = ce_dist(xyz, a + i, a + j);
}

__global__ void __launch_bounds__(kBlock) k_ce_similarity(const double* __restrict__ wa, const double* __restrict__ wb, const CePair* __restrict__ pairs,
                                                          long long n_pairs, double* __restrict__ S) {
    __shared__ double rows[2][kTile][kTerms];
    const long long p = ce_find<&CePair::tlo>(pairs, n_pairs, (long long)blockIdx.x);
    const CePair q = pairs[p];
    const int ra = (int)q.ma - kW + 1, rb = (int)q.mb - kW + 1;        // both >= 1: the pair has tiles
    const int tiles_b = (rb + kTile - 1) / kTile;
    const int tile = (int)((long long)blockIdx.x - q.tlo);
    const int a0 = tile / tiles_b * kTile, b0 = tile % tiles_b * kTile;
    for (int i = threadIdx.x; i < 2 * kTile * kTerms; i += kBlock) {
        const int side = i / (kTile * kTerms), r = i / kTerms % kTile, t = i % kTerms;
        const int w = (side ? b0 : a0) + r;
        if (w < (side ? rb : ra)) rows[side][r][t] = side ? wb[kTerms * (q.rblo + w) + t] : wa[kTerms * (q.ralo + w) + t];
    }
    __syncthreads();
    const int i = threadIdx.x / kTile, j = threadIdx.x % kTile;
    if (a0 + i >= ra || b0 + j >= rb) return;
    double sum = 0.0;
#pragma unroll
    for (int t = 0; t < kTerms; ++t) sum += fabs(rows[0][i][t] - rows[1][j][t]);
    S[q.wlo + (long long)(a0 + i) * rb + (b0 + j)] = sum / (double)kTerms;
}

// D((ai, bi), (aj, bj)) of the rule: the 8 terms in its order
__device__ inline double ce_fragment_distance(const double* __restrict__ A, const double* __restrict__ B, int ai, int bi, int aj, int bj) {
    double sum = fabs(ce_dist(A, ai, aj) - ce_dist(B, bi, bj));
    sum += fabs(ce_dist(A, ai + kW - 1, aj + kW - 1) - ce_dist(B, bi + kW - 1, bj + kW - 1));
#pragma unroll
    for (int k = 1; k < kW - 1; ++k) sum += fabs(ce_dist(A, ai + k, aj + kW - 1 - k) - ce_dist(B, bi + k, bj + kW - 1 - k));
    return sum / (double)kW;
}

// The path from start (a0, b0), whose S is below d0: returns its number of AFPs and its score; with kKeep the AFPs go to `kept`
// ((a << 16) | b, at most kMaxAfps of them).  Every lane of the wavefront is here and every lane returns the same values.
template <bool kKeep>
__device__ inline int ce_trace(const double* __restrict__ A, const double* __restrict__ B, const double* __restrict__ S, int ra, int rb, int a0,
                               int b0, double d0, double d1, int gap_max, int lane, double& score, int* kept) {
    int path[kPathRegs] = {0, 0, 0, 0};
    if (lane == 0) path[0] = (a0 << 16) | b0;
    int n = 1, a = a0, b = b0;
    double sum_s = S[(long long)a0 * rb + b0], sum_d = 0.0;
    const int g = lane;
    const int step_a = (g & 1) ? (g + 1) / 2 : 0, step_b = (g & 1) ? 0 : g / 2;
    const double inf = __builtin_inf();
    while (n < kMaxAfps) {
        const int ca = a + kW + step_a, cb = b + kW + step_b;
        bool ok = g <= 2 * gap_max && ca < ra && cb < rb;
        const double s_cand = ok ? S[(long long)ca * rb + cb] : inf;
        ok = ok && s_cand < d0;
        const int sa = ok ? ca : 0, sb = ok ? cb : 0;
        double s = 0.0;
#pragma unroll
        for (int r = 0; r < kPathRegs; ++r) {
            const int here = n - kWave * r < kWave ? n - kWave * r : kWave;           // AFPs of the path in this register: uniform
            for (int k = 0; k < here; ++k) {
                const int afp = __shfl(path[r], k, kWave);                             // every lane takes part
                if (ok) s += ce_fragment_distance(A, B, afp >> 16, afp & 0xffff, sa, sb);
            }
        }
        const double c = s / (double)n;
        const bool eligible = ok && c < d1;
        double cost = eligible ? c : inf;
        int chosen = eligible ? g : kWave;
        for (int m = kWave / 2; m >= 1; m >>= 1) {                                     // the smallest c, of equal ones the smallest g
            const double oc = __shfl_xor(cost, m, kWave);
            const int og = __shfl_xor(chosen, m, kWave);
            if (oc < cost || (oc == cost && og < chosen)) {
                cost = oc;
                chosen = og;
            }
        }
        if (chosen >= kWave) break;                                                    // uniform: every lane holds the same (cost, chosen)
        const double s_new = __shfl(s_cand, chosen, kWave), d_new = __shfl(s, chosen, kWave);
        const int na = __shfl(ca, chosen, kWave), nb = __shfl(cb, chosen, kWave);
        const double grown = ((sum_s + s_new) + (sum_d + d_new)) / (double)((n + 1) + (n + 1) * n / 2);
        if (!(grown < d1)) break;
#pragma unroll
        for (int r = 0; r < kPathRegs; ++r)
            if (r == n / kWave && lane == n % kWave) path[r] = (na << 16) | nb;
        sum_s += s_new;
        sum_d += d_new;
        a = na;
        b = nb;
        ++n;
    }
    score = (sum_s + sum_d) / (double)(n + n * (n - 1) / 2);
    if (kKeep) {
#pragma unroll
        for (int r = 0; r < kPathRegs; ++r)
            if (kWave * r + lane < n) kept[kWave * r + lane] = path[r];
    }
    return n;
}

__global__ void __launch_bounds__(kBlock) k_ce_paths(const double* __restrict__ ca, const double* __restrict__ cb, const CePair* __restrict__ pairs,
                                                     long long n_pairs, long long n_windows, const double* __restrict__ S, double d0, double d1,
                                                     int gap_max, int* __restrict__ path_len, double* __restrict__ path_score) {
    const long long w = (long long)blockIdx.x * kPerBlock + threadIdx.x / kWave;
    if (w >= n_windows) return;                                        // the whole wavefront leaves: nothing below is a workgroup barrier
    const int lane = threadIdx.x % kWave;
    if (!(S[w] < d0)) {                                                // not a start
        if (lane == 0) path_len[w] = 0;
        return;
    }
    const CePair q = pairs[ce_find<&CePair::wlo>(pairs, n_pairs, w)];
    const int ra = (int)q.ma - kW + 1, rb = (int)q.mb - kW + 1;
    const int local = (int)(w - q.wlo);
    double score;
    const int n = ce_trace<false>(ca + 3 * q.calo, cb + 3 * q.cblo, S + q.wlo, ra, rb, local / rb, local % rb, d0, d1, gap_max, lane, score, nullptr);
    if (lane == 0) {
        path_len[w] = n;
        path_score[w] = score;
    }
}

// (length, score, index) of one start before another in candidate order
__device__ inline bool ce_before(int l1, double s1, int i1, int l2, double s2, int i2) {
    return l1 > l2 || (l1 == l2 && (s1 < s2 || (s1 == s2 && i1 < i2)));
}

__global__ void __launch_bounds__(kWave) k_ce_best(const double* __restrict__ ca, const double* __restrict__ cb, const int* __restrict__ orig_a,
                                                   const int* __restrict__ orig_b, const CePair* __restrict__ pairs, const double* __restrict__ S,
                                                   const int* __restrict__ path_len, const double* __restrict__ path_score, double d0, double d1,
                                                   int gap_max, int* __restrict__ align_out, double* __restrict__ score_out,
                                                   long long* __restrict__ count_out, double* __restrict__ transform_out) {
    __shared__ int traced[kMaxAfps], winner[kMaxAfps];
    __shared__ int aligned[TH_CE_MAX_POSITIONS];
    const long long pair = blockIdx.x;
    const int lane = threadIdx.x;
    const CePair q = pairs[pair];
    const int ra = q.ma >= kW ? (int)q.ma - kW + 1 : 0, rb = q.mb >= kW ? (int)q.mb - kW + 1 : 0;
    const int n_windows = ra * rb;                                     // at most 2041^2
    const double* A = ca + 3 * q.calo;
    const double* B = cb + 3 * q.cblo;
    const int* len = path_len + q.wlo;
    const double* sc = path_score + q.wlo;
    int n_starts = 0;
    for (int w = lane; w < n_windows; w += kWave) n_starts += len[w] > 0 ? 1 : 0;
    n_starts = wave_sum(n_starts);
    const int n_cand = n_starts < TH_CE_KEEP ? n_starts : TH_CE_KEEP;

    const double nan = __builtin_nan("");
    Fit best_fit;
    double best_rmsd = nan, best_score = nan;
    int best_n = 0;
    int prev_len = INT_MAX, prev_at = -1;                              // the candidate taken last: before every start
    double prev_score = -__builtin_inf();
    for (int c = 0; c < n_cand; ++c) {
        // the first start, in candidate order, after the one taken last
        int top_len = 0, top_at = INT_MAX;
        double top_score = __builtin_inf();
        for (int w = lane; w < n_windows; w += kWave) {
            const int l = len[w];
            if (l <= 0) continue;
            const double s = sc[w];
            if (ce_before(prev_len, prev_score, prev_at, l, s, w) && ce_before(l, s, w, top_len, top_score, top_at)) {
                top_len = l;
                top_score = s;
                top_at = w;
            }
        }
        for (int m = kWave / 2; m >= 1; m >>= 1) {
            const int ol = __shfl_xor(top_len, m, kWave), oa = __shfl_xor(top_at, m, kWave);
            const double os = __shfl_xor(top_score, m, kWave);
            if (ce_before(ol, os, oa, top_len, top_score, top_at)) {
                top_len = ol;
                top_score = os;
                top_at = oa;
            }
        }
        prev_len = top_len;
        prev_score = top_score;
        prev_at = top_at;
        // its path again, and the fit of th_superpose over its 8 n position pairs
        double score;
        const int n = ce_trace<true>(A, B, S + q.wlo, ra, rb, top_at / rb, top_at % rb, d0, d1, gap_max, lane, score, traced);
        __syncthreads();
        // Every sum runs over the pairs in path order, one after the other, as the rule has it: the RMSDs of near-identical
        // candidates differ by rounding alone, and the order of addition decides among them.  Every lane forms the same sums itself
        // (the loads are one address per wave); 20 candidates of at most 2048 pairs are nothing beside the paths.
        const int count = kW * n;
        const auto ref_at = [&](int i) { return A + 3 * ((traced[i / kW] >> 16) + i % kW); };          // position pair i of the path:
        const auto mob_at = [&](int i) { return B + 3 * ((traced[i / kW] & 0xffff) + i % kW); };       // its reference and its mobile side
        Fit fit;
        double sr[3] = {0.0, 0.0, 0.0}, sm[3] = {0.0, 0.0, 0.0};
        for (int i = 0; i < count; ++i) add_position(ref_at(i), mob_at(i), sr, sm);
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            fit.cm[x] = sm[x] / (double)count;
            fit.cr[x] = sr[x] / (double)count;
        }
        double C[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
        for (int i = 0; i < count; ++i) add_covariance(fit, ref_at(i), mob_at(i), C);
        double (&F)[9] = fit.R;                                        // this candidate's rotation
        horn_rotation(C, F);
        double sq = 0.0;
        for (int i = 0; i < count; ++i) {
            const double d = distance(fit, ref_at(i), mob_at(i));
            sq += d * d;
        }
        const double rmsd = sqrt(sq / (double)count);
        if (c == 0 || rmsd < best_rmsd) {                              // uniform: of equal RMSDs the first candidate stays
            best_rmsd = rmsd;
            best_score = score;
            best_n = n;
            best_fit = fit;
            for (int k = lane; k < n; k += kWave) winner[k] = traced[k];
        }
        __syncthreads();
    }

    for (int i = lane; i < (int)q.na; i += kWave) aligned[i] = -1;
    __syncthreads();
    for (int i = lane; i < kW * best_n; i += kWave) {
        const int afp = winner[i / kW];
        aligned[orig_a[q.calo + (afp >> 16) + i % kW]] = orig_b[q.cblo + (afp & 0xffff) + i % kW];
    }
    __syncthreads();
    for (int i = lane; i < (int)q.na; i += kWave) align_out[q.alo + i] = aligned[i];
    if (lane != 0) return;
    score_out[2 * pair] = best_rmsd;
    score_out[2 * pair + 1] = best_score;
    long long* count = count_out + 6 * pair;
    count[0] = q.ma;
    count[1] = q.mb;
    count[2] = n_starts;
    count[3] = best_n;
    count[4] = kW * best_n;
    count[5] = n_cand;
    if (transform_out) store(best_fit, transform_out + 12 * pair);     // the identity when there is no start
}

// offsets of one of the two lists: from 0 to total, never decreasing, no structure above the limit
int ce_check_offsets(const char* side, const char* name, const char* total_name, const int64_t* offsets, int64_t total, int64_t n_pairs) {
    if (int rc = th_check_offsets("th_cealign", name, total_name, offsets, n_pairs, total)) return rc;
    for (int64_t p = 0; p < n_pairs; ++p)
        if (offsets[p + 1] - offsets[p] > TH_CE_MAX_POSITIONS)
            TH_FAIL(TH_EINVAL, "th_cealign: %s structure %lld has %lld positions (limit TH_CE_MAX_POSITIONS = %d)", side, (long long)p,
                    (long long)(offsets[p + 1] - offsets[p]), TH_CE_MAX_POSITIONS);
    return TH_OK;
}

// the valid positions of one structure, appended to the compacted list with their local original indices
long long ce_compact(const double* xyz, long long lo, long long n, std::vector<double>& out, std::vector<int>& orig) {
    long long m = 0;
    for (long long i = 0; i < n; ++i) {
        const double* r = xyz + 3 * (lo + i);
        if (finite3(r)) {
            out.insert(out.end(), r, r + 3);
            orig.push_back((int)i);
            ++m;
        }
    }
    return m;
}

}  // namespace

extern "C" int th_cealign(int device, const double* ref_xyz, int64_t ref_total, const int64_t* ref_offsets, const double* mob_xyz, int64_t mob_total,
                          const int64_t* mob_offsets, int64_t n_pairs, double d0, double d1, int gap_max, int32_t* align_out, double* score_out,
                          int64_t* count_out, double* transform_out, double* kernel_ms) {
    if (ref_total < 0 || mob_total < 0 || n_pairs < 0)
        TH_FAIL(TH_EINVAL, "th_cealign: negative size (ref_total = %lld, mob_total = %lld, n_pairs = %lld)", (long long)ref_total, (long long)mob_total,
                (long long)n_pairs);
    if (ref_total > INT_MAX || mob_total > INT_MAX || n_pairs > INT_MAX)
        TH_FAIL(TH_EINVAL, "th_cealign: %lld + %lld positions / %lld pairs in one call (limit 2^31 - 1 each)", (long long)ref_total, (long long)mob_total,
                (long long)n_pairs);
    if (!std::isfinite(d0) || d0 <= 0.0) TH_FAIL(TH_EINVAL, "th_cealign: d0 = %g is not a positive finite number", d0);
    if (!std::isfinite(d1) || d1 <= 0.0) TH_FAIL(TH_EINVAL, "th_cealign: d1 = %g is not a positive finite number", d1);
    if (gap_max < 0 || 2 * gap_max + 1 > kWave)
        TH_FAIL(TH_EINVAL, "th_cealign: gap_max = %d is outside 0 .. 31 (its 2 gap_max + 1 candidates are the lanes of one wavefront)", gap_max);
    if (n_pairs == 0) {
        if (ref_total != 0 || mob_total != 0)
            TH_FAIL(TH_EINVAL, "th_cealign: n_pairs = 0 owns no position, ref_total = %lld, mob_total = %lld", (long long)ref_total, (long long)mob_total);
        if (kernel_ms) *kernel_ms = 0.0;
        return TH_OK;
    }
    if (!ref_offsets || !mob_offsets || !score_out || !count_out || (ref_total > 0 && (!ref_xyz || !align_out)) || (mob_total > 0 && !mob_xyz))
        TH_FAIL(TH_EINVAL, "th_cealign: n_pairs = %lld needs ref_offsets, mob_offsets, score_out and count_out, ref_total = %lld needs ref_xyz and "
                           "align_out, mob_total = %lld needs mob_xyz", (long long)n_pairs, (long long)ref_total, (long long)mob_total);
    if (int rc = ce_check_offsets("ref", "ref_offsets", "ref_total", ref_offsets, ref_total, n_pairs)) return rc;
    if (int rc = ce_check_offsets("mob", "mob_offsets", "mob_total", mob_offsets, mob_total, n_pairs)) return rc;

    const size_t np = (size_t)n_pairs, nr = (size_t)ref_total;
    std::vector<CePair> pairs;
    std::vector<double> ca, cb;
    std::vector<int> orig_a, orig_b;
    long long rows_a = 0, rows_b = 0, n_windows = 0, n_tiles = 0;
    try {
        pairs.resize(np + 1);
        ca.reserve(3 * nr);
        cb.reserve(3 * (size_t)mob_total);
        for (size_t p = 0; p < np; ++p) {
            CePair& q = pairs[p];
            q.alo = ref_offsets[p];
            q.na = ref_offsets[p + 1] - ref_offsets[p];
            q.blo = mob_offsets[p];
            q.nb = mob_offsets[p + 1] - mob_offsets[p];
            q.calo = (long long)orig_a.size();
            q.cblo = (long long)orig_b.size();
            q.ma = ce_compact(ref_xyz, q.alo, q.na, ca, orig_a);
            q.mb = ce_compact(mob_xyz, q.blo, q.nb, cb, orig_b);
            q.ralo = rows_a;
            q.rblo = rows_b;
            q.wlo = n_windows;
            q.tlo = n_tiles;
            if (q.ma >= kW && q.mb >= kW) {                            // otherwise the pair has no window start at all
                const long long ra = q.ma - kW + 1, rb = q.mb - kW + 1;
                rows_a += ra;
                rows_b += rb;
                n_windows += ra * rb;
                n_tiles += ((ra + kTile - 1) / kTile) * ((rb + kTile - 1) / kTile);
            }
        }
        pairs[np] = CePair{ref_total, 0, mob_total, 0, (long long)orig_a.size(), 0, (long long)orig_b.size(), 0, rows_a, rows_b, n_windows, n_tiles};
    } catch (const std::bad_alloc&) {
        TH_FAIL(TH_ENOMEM, "th_cealign: out of host memory for the valid positions of %lld + %lld positions", (long long)ref_total, (long long)mob_total);
    }
    if ((n_windows + kPerBlock - 1) / kPerBlock > INT_MAX)
        TH_FAIL(TH_EINVAL, "th_cealign: %lld window pairs in one call (limit 2^33 - 4): submit fewer pairs at once", n_windows);
    const size_t nca = orig_a.size(), ncb = orig_b.size(), nw = (size_t)n_windows;

    ThLayout lay;
    const size_t o_ca = lay.take(nca * 3 * sizeof(double)), o_cb = lay.take(ncb * 3 * sizeof(double));
    const size_t o_oa = lay.take(nca * sizeof(int)), o_ob = lay.take(ncb * sizeof(int)), o_pairs = lay.take((np + 1) * sizeof(CePair));
    const size_t o_wa = lay.take((size_t)rows_a * kTerms * sizeof(double)), o_wb = lay.take((size_t)rows_b * kTerms * sizeof(double));
    const size_t o_s = lay.take(nw * sizeof(double)), o_len = lay.take(nw * sizeof(int)), o_ps = lay.take(nw * sizeof(double));
    const size_t o_align = lay.take(nr * sizeof(int32_t)), o_score = lay.take(np * 2 * sizeof(double)), o_count = lay.take(np * 6 * sizeof(int64_t));
    const size_t o_tr = lay.take(transform_out ? np * 12 * sizeof(double) : 0);
    ThCall call;
    if (int rc = call.open("th_cealign", device, lay.bytes, kernel_ms ? 2 : 0)) return rc;
    double *d_ca = call.at<double>(o_ca), *d_cb = call.at<double>(o_cb), *d_wa = call.at<double>(o_wa), *d_wb = call.at<double>(o_wb);
    double *d_s = call.at<double>(o_s), *d_ps = call.at<double>(o_ps), *d_score = call.at<double>(o_score);
    double* d_tr = transform_out ? call.at<double>(o_tr) : nullptr;
    int *d_oa = call.at<int>(o_oa), *d_ob = call.at<int>(o_ob), *d_len = call.at<int>(o_len), *d_align = call.at<int>(o_align);
    CePair* d_pairs = call.at<CePair>(o_pairs);
    long long* d_count = call.at<long long>(o_count);
    hipStream_t st = call.st[0];
    if (nca) {
        HIP_TRY(hipMemcpyAsync(d_ca, ca.data(), nca * 3 * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_oa, orig_a.data(), nca * sizeof(int), hipMemcpyHostToDevice, st));
    }
    if (ncb) {
        HIP_TRY(hipMemcpyAsync(d_cb, cb.data(), ncb * 3 * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_ob, orig_b.data(), ncb * sizeof(int), hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipMemcpyAsync(d_pairs, pairs.data(), (np + 1) * sizeof(CePair), hipMemcpyHostToDevice, st));
    HIP_TRY(call.mark(0));
    if (nw) {
        hipLaunchKernelGGL(k_ce_windows, dim3((unsigned)((rows_a + rows_b + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, d_ca, d_cb, d_pairs,
                           (long long)n_pairs, rows_a, rows_b, d_wa, d_wb);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_ce_similarity, dim3((unsigned)n_tiles), dim3(kBlock), 0, st, d_wa, d_wb, d_pairs, (long long)n_pairs, d_s);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_ce_paths, dim3((unsigned)((n_windows + kPerBlock - 1) / kPerBlock)), dim3(kBlock), 0, st, d_ca, d_cb, d_pairs,
                           (long long)n_pairs, n_windows, d_s, d0, d1, gap_max, d_len, d_ps);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_ce_best, dim3((unsigned)np), dim3(kWave), 0, st, d_ca, d_cb, d_oa, d_ob, d_pairs, d_s, d_len, d_ps, d0, d1, gap_max, d_align,
                       d_score, d_count, d_tr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(call.mark(1));
    if (nr) HIP_TRY(hipMemcpyAsync(align_out, d_align, nr * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(score_out, d_score, np * 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(count_out, d_count, np * 6 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (transform_out) HIP_TRY(hipMemcpyAsync(transform_out, d_tr, np * 12 * sizeof(double), hipMemcpyDeviceToHost, st));
    return call.finish(kernel_ms);
}
