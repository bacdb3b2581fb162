// th_seqalign: the sequence alignment of every model to its native — global with affine gap costs, the end gaps free or charged
// (Gotoh's three tables H, E, F) — for a BATCH of (reference, model) pairs in one call.  A residue is one byte (0..19 the letters
// ACDEFGHIKLMNPQRSTVWY, 20 any other), the substitution table is an input, everything is an integer.  The rule is written out in
// include/timed_hip.h.  *** PARITY UNPINNED AGAINST PYMOL ***: this stands where the reference calls cmd.align, whose recurrences, end-gap
// treatment and tie handling are not available to pin against; the rule is this project's own.
//
// k_seqalign_fill, the hot path: one wavefront per pair.  The model's columns are cut into panels of 64 strips of kStrip = 8 columns;
// lane l owns strip l of the panel and works on reference row t - l at step t (a skewed pipeline), so the 64 lanes sit on one
// anti-diagonal of strips.  A lane keeps H and F of the row above for its 8 columns in registers; the H and E of its strip's right edge
// go to lane l + 1, with the row's residue, by a cross-lane move (no LDS traffic, no barrier).  The 8 scores S[a_i][b_j] of a strip come from ONE 8-byte
// LDS read of the lane's "profile" — for each of the 21 codes the strip's 8 scores as bytes (a table entry is within +-127),
// laid out [code][lane] so that the 64 reads of a step fall on distinct banks whatever the codes are.  Lane 0 takes its left edge from
// the border (first panel) or from the edge column the previous panel's lane 63 left in memory; it and the row's residue are fetched 64
// rows at a time, one row per lane, and handed to lane 0 by v_readlane.  The four trace bits of a cell — origin (diagonal / F / E),
// E extended, F extended — make one dword per (row, strip), stored in step order [panel][t][lane]: the 64 stores of a step are one
// contiguous line.  The last row and the last column of H are left for the trace kernel.
// k_seqalign_trace: one thread per pair finds the end cell (the last row and column, in the order of the rule), walks the bits back,
// writes align_out (every reference position exactly once) and the eight counts.  A step of the walk depends on the bits of the one
// before: the thread fetches 8 rows of two strips at once into a window of its own in LDS and walks there until the path leaves it.  Pairs with an empty side are finished here alone.
// All integers, no atomics, no float arithmetic; a pair reads and writes only its own slices, so its bytes do not depend on its place.
#include <hip/hip_runtime.h>

#include <climits>
#include <new>
#include <vector>

#include "common.h"
#include "oneshot.h"

// 1: a strip's right edge goes to the next lane by one DPP move (wave_shr:1); 0: by __shfl_up (ds_bpermute_b32) — the same integers,
// a timing build (profiles/seqalign.txt)
#ifndef TH_SEQALIGN_DPP
#define TH_SEQALIGN_DPP 1
#endif

namespace {

constexpr int kWave = 64;
constexpr int kStrip = 8;                      // columns per lane: their trace bits are one dword
constexpr int kPanel = kWave * kStrip;         // columns per panel
constexpr int kCodes = 21;
constexpr int kWindowRows = 8;                 // k_seqalign_trace: rows of trace bits a thread fetches at a time, of two strips
constexpr int kWindowStride = 2 * kWindowRows + 1;      // odd: the threads' windows start on distinct LDS banks
constexpr int kNeg = -(1 << 30);               // "minus infinity"
constexpr int kMaxLength = TH_SEQALIGN_MAX_LENGTH;
constexpr long long kMax = 2147483647LL;

struct SaPair {
    long long ref0, mob0;      // first residue of either sequence
    long long trace0;          // first dword of the trace bits
    long long ints0;           // first int of: edge H [n + 1], edge E [n + 1], last row [m + 1], last column [n + 1]
    int n, m;
};

// dwords of trace bits of an n x m pair: [panel][t = row + lane][lane], a whole panel 64 lanes wide, the last as wide as it has strips
__host__ __device__ inline long long trace_words(int n, int m) {
    if (n == 0 || m == 0) return 0;
    const int panels = (m + kPanel - 1) / kPanel;
    const int nl = (m - (panels - 1) * kPanel + kStrip - 1) / kStrip;
    return (long long)(panels - 1) * (n + kWave - 1) * kWave + (long long)(n + nl - 1) * nl;
}

// the value of lane l - 1 (lane 0 keeps its own, which its caller replaces)
__device__ __forceinline__ int shift_up(int v) {
#if TH_SEQALIGN_DPP
    return __builtin_amdgcn_update_dpp(v, v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
#else
    return __shfl_up(v, 1, kWave);
#endif
}

__global__ void __launch_bounds__(kWave) k_seqalign_fill(const unsigned char* __restrict__ ref, const unsigned char* __restrict__ mob,
                                                         const SaPair* __restrict__ pairs, const signed char* __restrict__ table, int gap_open,
                                                         int gap_extend, int free_ends, unsigned* __restrict__ trace, int* __restrict__ ints) {
    __shared__ signed char tab[kCodes * kCodes + 7];
    __shared__ uint2 profile[kCodes * kWave];                       // [code][lane]: the lane's 8 scores against that code, one byte each
    const int lane = threadIdx.x;
    const SaPair P = pairs[blockIdx.x];
    const int n = P.n, m = P.m;
    if (n == 0 || m == 0) return;                                   // the whole wavefront: k_seqalign_trace finishes such a pair alone
    for (int k = lane; k < kCodes * kCodes; k += kWave) tab[k] = table[k];
    const unsigned char* a = ref + P.ref0;
    const unsigned char* b = mob + P.mob0;
    int* const edge_h = ints + P.ints0;
    int* const edge_e = edge_h + (n + 1);
    int* const last_row = edge_e + (n + 1);
    int* const last_col = last_row + (m + 1);
    const int panels = (m + kPanel - 1) / kPanel;
    for (int p = 0; p < panels; ++p) {
        const int c0 = p * kPanel, left = m - c0;
        const int nl = left >= kPanel ? kWave : (left + kStrip - 1) / kStrip;      // lanes that own a column
        const bool last = p == panels - 1;
        const int j0 = c0 + kStrip * lane;                          // the column left of the strip: it owns j0 + 1 .. j0 + 8
        int code[kStrip];
#pragma unroll
        for (int k = 0; k < kStrip; ++k) code[k] = j0 + k < m ? b[j0 + k] : 20;
        __syncthreads();                                            // the table is staged; the previous panel's profile is no longer read
        for (int c = 0; c < kCodes; ++c) {
            unsigned lo = 0, hi = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                lo |= (unsigned)(unsigned char)tab[c * kCodes + code[k]] << (8 * k);
                hi |= (unsigned)(unsigned char)tab[c * kCodes + code[k + 4]] << (8 * k);
            }
            profile[c * kWave + lane] = make_uint2(lo, hi);
        }
        __syncthreads();
        int h_up[kStrip], f_up[kStrip];                             // H and F of the row above
#pragma unroll
        for (int k = 0; k < kStrip; ++k) {
            h_up[k] = free_ends ? 0 : -(gap_open + (j0 + k) * gap_extend);
            f_up[k] = kNeg;
        }
        int diag = (free_ends || j0 == 0) ? 0 : -(gap_open + (j0 - 1) * gap_extend);       // H[0][j0]
        int h_out = 0, e_out = kNeg, a_cur = 0;                     // the right edge of the row just done, and that row's residue
        int block_h = 0, block_e = kNeg, block_a = 0;               // lane q: edge and residue of row t0 + q + 1, t0 the last multiple of 64
        unsigned* const tr = trace + P.trace0 + (long long)p * (n + kWave - 1) * kWave;
        const int lane_m = last ? (m - 1 - c0) / kStrip : -1, k_m = (m - 1 - c0) % kStrip;    // who owns column m
        const int steps = n + nl - 1;
        for (int t0 = 0; t0 < steps; t0 += kWave) {                 // 64 steps a block: the loads stay out of the step loop, which only stores
            {
                const int r = t0 + lane;                            // row r + 1
                block_a = r < n ? a[r] : 0;
                if (p > 0) {
                    block_h = r < n ? edge_h[r + 1] : 0;
                    block_e = r < n ? edge_e[r + 1] : kNeg;
                }
            }
            const int q_end = steps - t0 < kWave ? steps - t0 : kWave;
          for (int q = 0; q < q_end; ++q) {
            const int t = t0 + q;
            int h_left = shift_up(h_out), e_left = shift_up(e_out), a_row = shift_up(a_cur);
            const int a0 = __builtin_amdgcn_readlane(block_a, q), h0 = __builtin_amdgcn_readlane(block_h, q),
                      e0 = __builtin_amdgcn_readlane(block_e, q);
            if (lane == 0) {                                        // row t + 1
                a_row = a0;
                h_left = p > 0 ? h0 : (free_ends ? 0 : -(gap_open + t * gap_extend));
                e_left = p > 0 ? e0 : kNeg;
            }
            a_cur = a_row;
            const int i = t - lane + 1;
            if (lane < nl && i >= 1 && i <= n) {
                const uint2 scores = profile[a_cur * kWave + lane];
                unsigned word = 0;
                int d = diag, hl = h_left, el = e_left;
#pragma unroll
                for (int k = 0; k < kStrip; ++k) {
                    const int s = (int)((k < 4 ? scores.x : scores.y) << (24 - 8 * (k & 3))) >> 24;
                    const int e_open = hl - gap_open, e_ext = el - gap_extend;
                    const int e = e_ext > e_open ? e_ext : e_open;
                    const int f_open = h_up[k] - gap_open, f_ext = f_up[k] - gap_extend;
                    const int f = f_ext > f_open ? f_ext : f_open;
                    int h = d + s;
                    unsigned bits = 0;
                    if (f > h) { h = f; bits = 1; }
                    if (e > h) { h = e; bits = 2; }
                    bits |= (e_ext > e_open ? 4u : 0u) | (f_ext > f_open ? 8u : 0u);
                    word |= bits << (4 * k);
                    d = h_up[k];
                    h_up[k] = h;
                    f_up[k] = f;
                    hl = h;
                    el = e;
                }
                diag = h_left;
                h_out = hl;
                e_out = el;
                tr[t * nl + lane] = word;
                if (!last && lane == kWave - 1) {                   // the next panel's left edge; its row i was read at step i - 1 at the latest
                    edge_h[i] = hl;
                    edge_e[i] = el;
                }
                if (lane == lane_m) {
                    int hm = h_up[0];
#pragma unroll
                    for (int k = 1; k < kStrip; ++k) hm = k == k_m ? h_up[k] : hm;
                    last_col[i] = hm;
                }
                if (i == n) {
#pragma unroll
                    for (int k = 0; k < kStrip; ++k)
                        if (j0 + k < m) last_row[j0 + k + 1] = h_up[k];
                }
            }
          }
        }
        __threadfence();                                            // lane 63's edge column is visible to the next panel's block reads
    }
}

__global__ void __launch_bounds__(kWave) k_seqalign_trace(const unsigned char* __restrict__ ref, const unsigned char* __restrict__ mob,
                                                          const SaPair* __restrict__ pairs, long long n_pairs, const signed char* __restrict__ table,
                                                          int gap_open, int gap_extend, int free_ends, const unsigned* __restrict__ trace,
                                                          const int* __restrict__ ints, int* __restrict__ align_out, long long* __restrict__ count_out) {
    __shared__ unsigned window[kWave * kWindowStride];
    const long long pair = (long long)blockIdx.x * kWave + threadIdx.x;
    if (pair >= n_pairs) return;
    const SaPair P = pairs[pair];
    const int n = P.n, m = P.m;
    int* const align = align_out + P.ref0;
    long long* const out = count_out + 8 * pair;
    out[0] = n;
    out[1] = m;
    if (n == 0 || m == 0) {
        for (int i = 0; i < n; ++i) align[i] = -1;
        const int longer = n > m ? n : m;
        out[2] = free_ends || longer == 0 ? 0 : -(long long)(gap_open + (longer - 1) * gap_extend);
        for (int c = 3; c < 8; ++c) out[c] = 0;
        return;
    }
    const unsigned char* a = ref + P.ref0;
    const unsigned char* b = mob + P.mob0;
    const int* const last_row = ints + P.ints0 + 2 * (n + 1);
    const int* const last_col = last_row + (m + 1);
    int end_i = n, end_j = m, score = last_row[m];
    if (free_ends) {                                                // (n, m), then the last row leftwards, then the last column upwards
#pragma unroll 8
        for (int j = m - 1; j >= 0; --j) {
            const int v = j > 0 ? last_row[j] : 0;
            if (v > score) { score = v; end_i = n; end_j = j; }
        }
#pragma unroll 8
        for (int i = n - 1; i >= 0; --i) {
            const int v = i > 0 ? last_col[i] : 0;
            if (v > score) { score = v; end_i = i; end_j = m; }
        }
    }
    for (int i = end_i; i < n; ++i) align[i] = -1;
    const int panels = (m + kPanel - 1) / kPanel;
    const int nl_last = (m - (panels - 1) * kPanel + kStrip - 1) / kStrip;
    const unsigned* const tr = trace + P.trace0;
    // a thread's window on the bits: rows win_i - 7 .. win_i of strips win_s and win_s - 1, fetched by 16 loads at once when the path
    // leaves it — a path climbs a row per step at most, and the rows above are where it goes
    unsigned* const win = window + threadIdx.x * kWindowStride;
    int win_i = -1, win_s = -1;                                     // no row is above i >= 1: the first step fetches
    int i = end_i, j = end_j, state = 0;                            // 0 H, 1 F, 2 E
    int aligned = 0, identical = 0, positive = 0, gaps = 0, gap_residues = 0, next_i = 0, next_j = 0;      // the aligned pair met before this one
    while (i > 0 && j > 0) {
        const int strip = (j - 1) / kStrip;
        if (i > win_i || i <= win_i - kWindowRows || strip > win_s || strip < win_s - 1) {
            win_i = i;
            win_s = strip;
            unsigned fetched[2 * kWindowRows];
#pragma unroll
            for (int r = 0; r < kWindowRows; ++r)
#pragma unroll
                for (int d = 0; d < 2; ++d) {
                    const int row = i - r, sd = strip - d;
                    unsigned v = 0;
                    if (row >= 1 && sd >= 0) {
                        const int p = sd / kWave, l = sd % kWave, nl = p == panels - 1 ? nl_last : kWave;
                        v = tr[(long long)p * (n + kWave - 1) * kWave + (long long)(row - 1 + l) * nl + l];
                    }
                    fetched[2 * r + d] = v;
                }
#pragma unroll
            for (int k = 0; k < 2 * kWindowRows; ++k) win[k] = fetched[k];
        }
        const unsigned bits = (win[2 * (win_i - i) + (win_s - strip)] >> (4 * ((j - 1) % kStrip))) & 15u;
        if (state == 0) {
            const unsigned origin = bits & 3u;
            if (origin == 0) {
                align[i - 1] = j - 1;
                const int ca = a[i - 1], cb = b[j - 1];
                identical += ca == cb;
                positive += table[ca * kCodes + cb] > 0;
                if (aligned > 0) {                                  // the runs between this pair and the one after it
                    const int ref_run = next_i - i - 1, mob_run = next_j - j - 1;
                    gaps += (ref_run > 0) + (mob_run > 0);
                    gap_residues += ref_run + mob_run;
                }
                ++aligned;
                next_i = i;
                next_j = j;
                --i;
                --j;
            } else {
                state = (int)origin;
            }
        } else if (state == 1) {
            state = (bits & 8u) ? 1 : 0;
            align[i - 1] = -1;
            --i;
        } else {
            state = (bits & 4u) ? 2 : 0;
            --j;
        }
    }
    for (int r = 0; r < i; ++r) align[r] = -1;
    out[2] = score;
    out[3] = aligned;
    out[4] = identical;
    out[5] = positive;
    out[6] = gaps;
    out[7] = gap_residues;
}

}  // namespace

extern "C" int th_seqalign(int device, const uint8_t* ref_codes, int64_t ref_total, const int64_t* ref_offsets, const uint8_t* mob_codes,
                           int64_t mob_total, const int64_t* mob_offsets, int64_t n_pairs, const int32_t* matrix, int gap_open, int gap_extend,
                           int free_ends, int32_t* align_out, int64_t* count_out, double* kernel_ms) {
    if (ref_total < 0 || mob_total < 0 || n_pairs < 0)
        TH_FAIL(TH_EINVAL, "th_seqalign: negative size (ref_total = %lld, mob_total = %lld, n_pairs = %lld)", (long long)ref_total, (long long)mob_total,
                (long long)n_pairs);
    if (ref_total > kMax || mob_total > kMax || n_pairs > kMax)
        TH_FAIL(TH_EINVAL, "th_seqalign: ref_total = %lld, mob_total = %lld, n_pairs = %lld in one call (limit 2^31 - 1 each)", (long long)ref_total,
                (long long)mob_total, (long long)n_pairs);
    if (gap_extend < 0 || gap_open < gap_extend || gap_open > 32767)
        TH_FAIL(TH_EINVAL, "th_seqalign: gap_open = %d, gap_extend = %d: need 0 <= gap_extend <= gap_open <= 32767", gap_open, gap_extend);
    if (free_ends != 0 && free_ends != 1) TH_FAIL(TH_EINVAL, "th_seqalign: free_ends = %d is neither 0 nor 1", free_ends);
    if (n_pairs == 0) {
        if (ref_total != 0 || mob_total != 0)
            TH_FAIL(TH_EINVAL, "th_seqalign: n_pairs = 0 owns no residue, ref_total = %lld, mob_total = %lld", (long long)ref_total, (long long)mob_total);
        if (kernel_ms) kernel_ms[0] = kernel_ms[1] = 0.0;
        return TH_OK;
    }
    if (!ref_offsets || !mob_offsets || !matrix || !count_out || (ref_total > 0 && (!ref_codes || !align_out)) || (mob_total > 0 && !mob_codes))
        TH_FAIL(TH_EINVAL, "th_seqalign: n_pairs = %lld needs ref_offsets, mob_offsets, matrix and count_out; ref_total = %lld needs ref_codes and "
                "align_out, mob_total = %lld needs mob_codes", (long long)n_pairs, (long long)ref_total, (long long)mob_total);
    if (int rc = th_check_offsets("th_seqalign", "ref_offsets", "ref_total", ref_offsets, n_pairs, ref_total)) return rc;
    if (int rc = th_check_offsets("th_seqalign", "mob_offsets", "mob_total", mob_offsets, n_pairs, mob_total)) return rc;
    signed char table[kCodes * kCodes];
    for (int k = 0; k < kCodes * kCodes; ++k) {
        if (matrix[k] < -127 || matrix[k] > 127)
            TH_FAIL(TH_EINVAL, "th_seqalign: matrix[%d][%d] = %d is outside -127 .. 127", k / kCodes, k % kCodes, (int)matrix[k]);
        table[k] = (signed char)matrix[k];
    }
    std::vector<SaPair> pairs;
    try {
        pairs.resize((size_t)n_pairs);
    } catch (const std::bad_alloc&) {
        TH_FAIL(TH_ENOMEM, "th_seqalign: out of host memory for %lld pairs", (long long)n_pairs);
    }
    long long at_trace = 0, at_ints = 0;
    for (int64_t k = 0; k < n_pairs; ++k) {
        const int64_t n = ref_offsets[k + 1] - ref_offsets[k], m = mob_offsets[k + 1] - mob_offsets[k];
        if (n > kMaxLength || m > kMaxLength)
            TH_FAIL(TH_EINVAL, "th_seqalign: pair %lld has sequences of %lld and %lld residues, above %d", (long long)k, (long long)n, (long long)m,
                    kMaxLength);
        pairs[(size_t)k] = SaPair{ref_offsets[k], mob_offsets[k], at_trace, at_ints, (int)n, (int)m};
        at_trace += trace_words((int)n, (int)m);
        at_ints += 3 * (n + 1) + (m + 1);
    }
    for (int64_t k = 0; k < ref_total; ++k)
        if (ref_codes[k] > 20) TH_FAIL(TH_EINVAL, "th_seqalign: ref_codes[%lld] = %d, a code is at most 20", (long long)k, (int)ref_codes[k]);
    for (int64_t k = 0; k < mob_total; ++k)
        if (mob_codes[k] > 20) TH_FAIL(TH_EINVAL, "th_seqalign: mob_codes[%lld] = %d, a code is at most 20", (long long)k, (int)mob_codes[k]);

    const size_t np = (size_t)n_pairs, nr = (size_t)ref_total, nm = (size_t)mob_total;
    ThLayout lay;
    const size_t o_ref = lay.take(nr), o_mob = lay.take(nm), o_pairs = lay.take(np * sizeof(SaPair)), o_table = lay.take(sizeof(table));
    const size_t o_trace = lay.take((size_t)at_trace * sizeof(unsigned)), o_ints = lay.take((size_t)at_ints * sizeof(int));
    const size_t o_align = lay.take(nr * sizeof(int32_t)), o_count = lay.take(np * 8 * sizeof(int64_t));
    ThCall call;
    if (int rc = call.open("th_seqalign", device, lay.bytes, kernel_ms ? 3 : 0)) return rc;
    unsigned char *d_ref = call.at<unsigned char>(o_ref), *d_mob = call.at<unsigned char>(o_mob);
    SaPair* d_pairs = call.at<SaPair>(o_pairs);
    signed char* d_table = call.at<signed char>(o_table);
    unsigned* d_trace = call.at<unsigned>(o_trace);
    int *d_ints = call.at<int>(o_ints), *d_align = call.at<int>(o_align);
    long long* d_count = call.at<long long>(o_count);
    hipStream_t st = call.st[0];
    if (nr > 0) HIP_TRY(hipMemcpyAsync(d_ref, ref_codes, nr, hipMemcpyHostToDevice, st));
    if (nm > 0) HIP_TRY(hipMemcpyAsync(d_mob, mob_codes, nm, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_pairs, pairs.data(), np * sizeof(SaPair), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_table, table, sizeof(table), hipMemcpyHostToDevice, st));
    HIP_TRY(call.mark(0));
    hipLaunchKernelGGL(k_seqalign_fill, dim3((unsigned)np), dim3(kWave), 0, st, d_ref, d_mob, d_pairs, d_table, gap_open, gap_extend, free_ends, d_trace,
                       d_ints);
    HIP_TRY(hipGetLastError());
    HIP_TRY(call.mark(1));
    hipLaunchKernelGGL(k_seqalign_trace, dim3((unsigned)((np + kWave - 1) / kWave)), dim3(kWave), 0, st, d_ref, d_mob, d_pairs, (long long)n_pairs,
                       d_table, gap_open, gap_extend, free_ends, d_trace, d_ints, d_align, d_count);
    HIP_TRY(hipGetLastError());
    HIP_TRY(call.mark(2));
    if (nr > 0) HIP_TRY(hipMemcpyAsync(align_out, d_align, nr * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(count_out, d_count, np * 8 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    return call.finish(kernel_ms, 2);
}
