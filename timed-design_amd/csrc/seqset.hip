// th_seqset: what a SET of sampled sequences looks like — the N sequences drawn for one structure, all of one length L, one byte per
// residue (0..19 the letters ACDEFGHIKLMNPQRSTVWY, 20 any other letter).  Per sequence its identity, similarity and substitution score
// against the native, its matches M(i, j) summed over the other sequences, its nearest other sequence, the first sequence equal to it
// and its cluster; per position the count of every code (the sequence logo of the draws); per set the totals; on request the whole
// N x N matrix of M.  Every set of a batch in one call.  The rule is written out in include/timed_hip.h.
//
//     The clustering is the incremental scheme of CD-HIT-like tools in its plainest form — greedy, in input order, a sequence joins the
//     lowest-indexed representative it matches at min_matches positions or more — and is THIS PROJECT'S OWN RULE, NOT THEIR CODE: no
//     word filter, no length sorting, no alignment (the draws of one structure are position-paired by construction).
//
// k_seqset_pack: every sequence once more on the device, padded with zero bytes to whole dwords and dword-aligned, four residues per
// dword; the pairs and the cluster kernel read these.
// k_seqset_pairs, the hot path: a work item is (set, a tile of kRows sequences i).  The sequences j of the set stream past it through LDS
// in tiles of kCols, both tiles staged kChunk positions at a time as packed dwords (row stride kChunk / 4 + 4 dwords: the 16-byte reads
// of a wavefront then fall on distinct banks).  A thread owns 4 x 4 pairs — rows ti + 16 a, columns tj + 16 b — and keeps their 16
// mismatch counts in registers.  Per dword x = a ^ b, mismatches += popcount((x + 0x7f7f7f7f) & 0x80808080) (add_mismatches, three
// instructions): a code is at most 20, so x < 0x80 in every byte, the addition carries into no neighbour and bit 7 of a byte is set exactly where the two codes differ
// (TH_SEQSET_PACKED 0 compares the four bytes one by one: the same integers).  Pad bytes and rows past the end are zero on both sides
// and cost nothing: M = L - mismatches.  When a column tile is finished the thread folds it into its rows' pair_sum, (nearest_matches,
// lowest j) and first_equal — its columns come in increasing j — and stores the matrix block if asked; at the end the 16 threads of a
// row meet through LDS, in thread order.  Both (i, j) and (j, i) are computed: the symmetry is not used.
// k_seqset_columns: a workgroup per (set, 16 positions); 16 threads per position walk every 16th sequence each, neighbouring threads
// read neighbouring bytes, and are summed in thread order (one thread per position leaves a set of 10 000 x 300 on two workgroups).
// A thread's 21 counts live in LDS: a register array indexed by the code would go to scratch.
// k_seqset_native: a wavefront per sequence, lanes over positions, the substitution table in LDS; three integer sums.
// k_seqset_cluster: one workgroup per set, sequences in order (csrc/pack_sidechains.hip is the precedent for one workgroup per item
// running a sequential search).  The representatives so far are shared out over the 1024 threads, in list order; each thread
// recomputes M(n, r) with the same packed compare and stops once the threshold is out of reach; a block minimum picks the lowest
// qualifying representative and ends the rounds.  Sets run in parallel across the device.
// k_seqset_totals: one wavefront per set, 64-bit integer sums of the per-sequence columns.
// All integers, no atomics; nothing depends on the grid, on arrival order, on a set's place in the batch or on matrix_out.
#include <hip/hip_runtime.h>

#include <climits>
#include <new>
#include <vector>

#include "common.h"
#include "device_math.h"
#include "oneshot.h"

// 1: four residues per compare (xor, add, and, popcount).  0: byte by byte — the same integers, a timing build (profiles/seqset.txt).
#ifndef TH_SEQSET_PACKED
#define TH_SEQSET_PACKED 1
#endif

// positions staged at a time by k_seqset_pairs, a multiple of 16.  256 is the product; 320 and 512 were measured against it
// (profiles/seqset.txt).
#ifndef TH_SEQSET_CHUNK
#define TH_SEQSET_CHUNK 256
#endif

namespace {

constexpr int kWave = 64;
constexpr int kRows = 64, kCols = 64;          // sequences per row tile and per column tile
constexpr int kChunk = TH_SEQSET_CHUNK;        // positions staged at a time
constexpr int kChunkWords = kChunk / 4;
constexpr int kStride = kChunkWords + 4;       // dwords between two staged sequences
constexpr int kThreads = 256;                  // 16 x 16 threads of 4 x 4 pairs
constexpr int kClusterThreads = 1024;          // k_seqset_cluster: representatives compared at a time
constexpr int kClusterWords = 16;              // and the dwords a thread compares between two looks at the threshold
static_assert(kChunk % 16 == 0 && (kRows + kCols) * kStride >= 4 * kRows * 16, "the staged tiles also hold the fold of a row's 16 threads");
constexpr int kCodes = 21;
constexpr int kPositions = 16, kSlices = kThreads / kPositions;      // k_seqset_columns: positions per workgroup, threads per position
constexpr int kSeqColumns = 8;
constexpr long long kMax = 2147483647LL;

struct SeqSet {
    long long seq0;        // the set's first sequence
    long long codes0;      // its first byte of codes
    long long words0;      // its first dword of the packed copy
    long long pos0;        // its first position (row of profile_out, byte of native)
    long long matrix0;     // its first entry of matrix_out
    int n, length, words;  // N, L, ceil(L / 4)
    int min_matches;       // -1: no clustering
};

// count += the number of bytes in which a and b differ.  Packed: three instructions a dword — v_xad_u32 is (a ^ b) + constant in one,
// v_bcnt_u32_b32 adds its popcount to the count it is given.  Written as instructions because the compiler, left alone, sums the
// popcounts of a thread's pairs in a tree of v_add3_u32 and does not always fuse the xor: 4.5 instructions a dword.
__device__ __forceinline__ void add_mismatches(int& count, unsigned a, unsigned b) {
#if TH_SEQSET_PACKED
    unsigned x;
    asm("v_xad_u32 %0, %1, %2, %3" : "=v"(x) : "v"(a), "v"(b), "s"(0x7f7f7f7fu));
    x &= 0x80808080u;
    asm("v_bcnt_u32_b32 %0, %1, %0" : "+v"(count) : "v"(x));
#else
    const unsigned x = a ^ b;
    count += ((x & 0xffu) != 0) + ((x & 0xff00u) != 0) + ((x & 0xff0000u) != 0) + ((x & 0xff000000u) != 0);
#endif
}

__global__ void __launch_bounds__(kThreads) k_seqset_pack(const unsigned char* __restrict__ codes, const SeqSet* __restrict__ sets,
                                                          const ThTile* __restrict__ items, unsigned* __restrict__ packed) {
    const ThTile it = items[blockIdx.x];
    const SeqSet s = sets[it.range];
    const int i0 = it.tile * kRows, rows = s.n - i0 < kRows ? s.n - i0 : kRows;
    const unsigned char* src = codes + s.codes0 + (long long)i0 * s.length;
    unsigned* dst = packed + s.words0 + (long long)i0 * s.words;
    const int total = rows * s.words;                               // rows <= N and N * L <= 2^31 - 1
    for (int k = threadIdx.x; k < total; k += kThreads) {
        const int r = k / s.words, w = k - r * s.words;
        const unsigned char* p = src + (long long)r * s.length + 4 * w;
        const int left = s.length - 4 * w;                          // 1 .. : the bytes of this dword that exist
        unsigned v = p[0];
        if (left > 1) v |= (unsigned)p[1] << 8;
        if (left > 2) v |= (unsigned)p[2] << 16;
        if (left > 3) v |= (unsigned)p[3] << 24;
        dst[k] = v;
    }
}

__global__ void __launch_bounds__(kThreads) k_seqset_pairs(const unsigned* __restrict__ packed, const SeqSet* __restrict__ sets,
                                                           const ThTile* __restrict__ items, int* __restrict__ seq_out,
                                                           int* __restrict__ matrix_out) {
    __shared__ __attribute__((aligned(16))) unsigned lds[(kRows + kCols) * kStride];
    unsigned* const A = lds;
    unsigned* const B = lds + kRows * kStride;
    const int tid = threadIdx.x, ti = tid / 16, tj = tid % 16;
    const ThTile it = items[blockIdx.x];
    const SeqSet s = sets[it.range];
    const int N = s.n, L = s.length, W = s.words, i0 = it.tile * kRows;
    const unsigned* base = packed + s.words0;
    const int chunks = (W + kChunkWords - 1) / kChunkWords;
    int pair_sum[4], best[4], best_j[4], first[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        pair_sum[a] = 0;
        best[a] = -1;
        best_j[a] = -1;
        first[a] = INT_MAX;
    }
    for (int j0 = 0; j0 < N; j0 += kCols) {
        int mism[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) mism[a][b] = 0;
        for (int c = 0; c < chunks; ++c) {
            const int w0 = c * kChunkWords;
            const int nw = W - w0 < kChunkWords ? W - w0 : kChunkWords;           // dwords of this chunk that exist
            const int nw4 = (nw + 3) & ~3;                                       // staged, the rest zero: the reads are 16 bytes wide
            const bool stage_rows = chunks > 1 || j0 == 0;                       // a single chunk of rows stays where it is
            if (c > 0 || j0 > 0) __syncthreads();                                // the previous chunk is no longer read
            for (int k = tid; k < kCols * nw4; k += kThreads) {
                const int r = k / nw4, w = k - r * nw4;
                const bool in = w < nw;
                const int i = i0 + r, j = j0 + r;
                if (stage_rows) A[r * kStride + w] = in && i < N ? base[(long long)i * W + w0 + w] : 0u;
                B[r * kStride + w] = in && j < N ? base[(long long)j * W + w0 + w] : 0u;
            }
            __syncthreads();
            for (int w = 0; w < nw4; w += 4) {
                uint4 ra[4], rb[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) ra[a] = *reinterpret_cast<const uint4*>(A + (ti + 16 * a) * kStride + w);
#pragma unroll
                for (int b = 0; b < 4; ++b) rb[b] = *reinterpret_cast<const uint4*>(B + (tj + 16 * b) * kStride + w);
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        add_mismatches(mism[a][b], ra[a].x, rb[b].x);
                        add_mismatches(mism[a][b], ra[a].y, rb[b].y);
                        add_mismatches(mism[a][b], ra[a].z, rb[b].z);
                        add_mismatches(mism[a][b], ra[a].w, rb[b].w);
                    }
            }
        }
        // the column tile is finished: this thread's columns j0 + tj + 16 b, in increasing order
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int i = i0 + ti + 16 * a;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int j = j0 + tj + 16 * b;
                if (i >= N || j >= N) continue;
                const int m = L - mism[a][b];
                if (m == L && first[a] == INT_MAX) first[a] = j;                 // the self pair counts
                if (j != i) {
                    pair_sum[a] += m;
                    if (m > best[a]) {
                        best[a] = m;
                        best_j[a] = j;
                    }
                }
                if (matrix_out) matrix_out[s.matrix0 + (long long)i * N + j] = m;
            }
        }
    }
    // the 16 threads of a row, in thread order
    __syncthreads();
    int* const fold = reinterpret_cast<int*>(lds);                               // [4][kRows][16]
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int at = (ti + 16 * a) * 16 + tj;
        fold[at] = pair_sum[a];
        fold[kRows * 16 + at] = best[a];
        fold[2 * kRows * 16 + at] = best_j[a];
        fold[3 * kRows * 16 + at] = first[a];
    }
    __syncthreads();
    if (tid < kRows && i0 + tid < N) {
        int sum = 0, m = -1, mj = -1, f = INT_MAX;
        for (int t = 0; t < 16; ++t) {
            const int at = tid * 16 + t;
            sum += fold[at];
            const int bm = fold[kRows * 16 + at], bj = fold[2 * kRows * 16 + at], bf = fold[3 * kRows * 16 + at];
            if (bm > m || (bm == m && bj >= 0 && bj < mj)) {
                m = bm;
                mj = bj;
            }
            f = bf < f ? bf : f;
        }
        int* out = seq_out + (s.seq0 + i0 + tid) * kSeqColumns;
        out[3] = sum;
        out[4] = m;
        out[5] = mj;
        out[6] = f;
    }
}

__global__ void __launch_bounds__(kThreads) k_seqset_columns(const unsigned char* __restrict__ codes, const SeqSet* __restrict__ sets,
                                                             const ThTile* __restrict__ items, int* __restrict__ profile_out) {
    __shared__ int counts[kThreads * kCodes];                                    // [slice][position][code]
    const int tid = threadIdx.x, slice = tid / kPositions, q = tid % kPositions;
    const ThTile it = items[blockIdx.x];                                         // positions tile * 16 ... of that set
    const SeqSet s = sets[it.range];
    const int p0 = it.tile * kPositions, pos = p0 + q;
    const int here = s.length - p0 < kPositions ? s.length - p0 : kPositions;
    for (int c = 0; c < kCodes; ++c) counts[tid * kCodes + c] = 0;               // 21 is odd: a thread's row starts on its own bank
    if (pos < s.length) {
        const unsigned char* p = codes + s.codes0 + pos;
        for (int n = slice; n < s.n; n += kSlices) counts[tid * kCodes + p[(long long)n * s.length]] += 1;
    }
    __syncthreads();
    int* out = profile_out + (s.pos0 + p0) * kCodes;
    for (int k = tid; k < here * kCodes; k += kThreads) {                        // k = position * 21 + code; the slices in order
        int sum = 0;
        for (int v = 0; v < kSlices; ++v) sum += counts[v * kPositions * kCodes + k];
        out[k] = sum;
    }
}

__global__ void __launch_bounds__(kThreads) k_seqset_native(const unsigned char* __restrict__ codes, const SeqSet* __restrict__ sets,
                                                            const ThTile* __restrict__ items, const unsigned char* __restrict__ native,
                                                            const signed char* __restrict__ substitution, int* __restrict__ seq_out) {
    __shared__ int table[400];
    const int tid = threadIdx.x, lane = tid % kWave;
    if (native)
        for (int k = tid; k < 400; k += kThreads) table[k] = substitution[k];
    __syncthreads();
    const ThTile it = items[blockIdx.x];
    const SeqSet s = sets[it.range];
    for (int r = tid / kWave; r < kRows; r += kThreads / kWave) {                // a wavefront per sequence
        const int i = it.tile * kRows + r;
        if (i >= s.n) break;
        int same = 0, similar = 0, score = 0;
        if (native) {
            const unsigned char* mine = codes + s.codes0 + (long long)i * s.length;
            const unsigned char* nat = native + s.pos0;
            for (int p = lane; p < s.length; p += kWave) {
                const int a = nat[p], b = mine[p];
                same += a == b;
                if (a < 20 && b < 20) {
                    const int v = table[a * 20 + b];
                    similar += v > 0;
                    score += v;
                }
            }
            same = wave_sum(same);
            similar = wave_sum(similar);
            score = wave_sum(score);
        }
        if (lane == 0) {
            int* out = seq_out + (s.seq0 + i) * kSeqColumns;
            out[0] = same;
            out[1] = similar;
            out[2] = score;
        }
    }
}

__global__ void __launch_bounds__(kClusterThreads) k_seqset_cluster(const unsigned* __restrict__ packed, const SeqSet* __restrict__ sets,
                                                             int* __restrict__ representatives, int* __restrict__ seq_out) {
    __shared__ int lowest[kClusterThreads / kWave];
    const int tid = threadIdx.x;
    const SeqSet s = sets[blockIdx.x];
    int* const out = seq_out + s.seq0 * kSeqColumns;
    if (s.min_matches < 0) {
        for (int n = tid; n < s.n; n += kClusterThreads) out[(long long)n * kSeqColumns + 7] = -1;
        return;
    }
    const unsigned* base = packed + s.words0;
    int* const reps = representatives + s.seq0;                                  // this set's representatives, in increasing order
    const int W = s.words, allowed = s.length - s.min_matches;                   // mismatches a member may have
    int n_reps = 0;                                                              // the same in every thread
    for (int n = 0; n < s.n; ++n) {
        const unsigned* mine = base + (long long)n * W;
        int found = INT_MAX;
        for (int k0 = 0; k0 < n_reps && found == INT_MAX; k0 += kClusterThreads) {
            int hit = INT_MAX;
            if (k0 + tid < n_reps) {
                const int r = reps[k0 + tid];
                const unsigned* theirs = base + (long long)r * W;
                int mism = 0;
                int w = 0;
                for (; w + kClusterWords <= W && mism <= allowed; w += kClusterWords) {      // 2 x 16 loads in flight, then the test
                    unsigned m[kClusterWords], t[kClusterWords];
#pragma unroll
                    for (int k = 0; k < kClusterWords; ++k) {
                        m[k] = mine[w + k];
                        t[k] = theirs[w + k];
                    }
#pragma unroll
                    for (int k = 0; k < kClusterWords; ++k) add_mismatches(mism, m[k], t[k]);
                }
                for (; w < W && mism <= allowed; ++w) add_mismatches(mism, mine[w], theirs[w]);
                if (mism <= allowed) hit = r;
            }
            for (int m = 32; m >= 1; m >>= 1) {
                const int other = __shfl_xor(hit, m, kWave);
                hit = other < hit ? other : hit;
            }
            __syncthreads();                                                     // the previous round's minima are no longer read
            if (tid % kWave == 0) lowest[tid / kWave] = hit;
            __syncthreads();
            for (int v = 0; v < kClusterThreads / kWave; ++v) found = lowest[v] < found ? lowest[v] : found;
        }
        if (tid == 0) {
            out[(long long)n * kSeqColumns + 7] = found == INT_MAX ? n : found;
            if (found == INT_MAX) reps[n_reps] = n;
        }
        if (found == INT_MAX) ++n_reps;
        __syncthreads();                                                         // the new representative is visible to the next sequence
    }
}

__global__ void __launch_bounds__(kThreads) k_seqset_totals(const SeqSet* __restrict__ sets, long long n_sets, const int* __restrict__ seq_out,
                                                            long long* __restrict__ set_out) {
    const long long k = (long long)blockIdx.x * (kThreads / kWave) + threadIdx.x / kWave;
    if (k >= n_sets) return;                   // the whole wavefront leaves
    const int lane = threadIdx.x % kWave;
    const SeqSet s = sets[k];
    long long pairs = 0, distinct = 0, clusters = 0, native = 0;
    for (int i = lane; i < s.n; i += kWave) {
        const int* row = seq_out + (s.seq0 + i) * kSeqColumns;
        native += row[0];
        pairs += row[3];
        distinct += row[6] == i;
        clusters += row[7] == i;
    }
    pairs = wave_sum(pairs);
    distinct = wave_sum(distinct);
    clusters = wave_sum(clusters);
    native = wave_sum(native);
    if (lane == 0) {
        set_out[4 * k] = pairs / 2;            // every pair was counted from both of its sequences
        set_out[4 * k + 1] = distinct;
        set_out[4 * k + 2] = s.min_matches < 0 ? -1 : clusters;
        set_out[4 * k + 3] = native;
    }
}

}  // namespace

extern "C" int th_seqset_tiles(int32_t* tiles_out) {
    if (!tiles_out) TH_FAIL(TH_EINVAL, "th_seqset_tiles: tiles_out is NULL");
    tiles_out[0] = kRows;
    tiles_out[1] = kCols;
    tiles_out[2] = kChunk;
    return TH_OK;
}

extern "C" int th_seqset(int device, const uint8_t* codes, int64_t total_codes, const int64_t* seq_offsets, const int32_t* lengths,
                         int64_t n_sets, const uint8_t* native, const int8_t* substitution, const int32_t* min_matches, int32_t* seq_out,
                         int32_t* profile_out, int32_t* matrix_out, int64_t* set_out, double* kernel_ms) {
    if (total_codes < 0 || n_sets < 0)
        TH_FAIL(TH_EINVAL, "th_seqset: negative size (total_codes = %lld, n_sets = %lld)", (long long)total_codes, (long long)n_sets);
    if (n_sets > kMax) TH_FAIL(TH_EINVAL, "th_seqset: n_sets = %lld in one call (limit 2^31 - 1)", (long long)n_sets);
    if (native && !substitution) TH_FAIL(TH_EINVAL, "th_seqset: native needs substitution, which is NULL");
    if (n_sets == 0) {
        if (total_codes != 0) TH_FAIL(TH_EINVAL, "th_seqset: n_sets = 0 owns no residue, total_codes = %lld", (long long)total_codes);
        if (kernel_ms) kernel_ms[0] = kernel_ms[1] = kernel_ms[2] = 0.0;
        return TH_OK;
    }
    if (!seq_offsets || !lengths || !set_out)
        TH_FAIL(TH_EINVAL, "th_seqset: n_sets = %lld needs seq_offsets, lengths and set_out", (long long)n_sets);
    if (seq_offsets[0] != 0 || seq_offsets[n_sets] < 0 || seq_offsets[n_sets] > kMax)
        TH_FAIL(TH_EINVAL, "th_seqset: seq_offsets run from %lld to %lld sequences, not from 0 to at most 2^31 - 1", (long long)seq_offsets[0],
                (long long)seq_offsets[n_sets]);
    const int64_t n_seq = seq_offsets[n_sets];
    if (int rc = th_check_offsets("th_seqset", "seq_offsets", "the number of sequences", seq_offsets, n_sets, n_seq)) return rc;
    std::vector<SeqSet> sets;
    std::vector<int64_t> pos_offsets;
    try {
        sets.resize((size_t)n_sets);
        pos_offsets.resize((size_t)n_sets + 1);
    } catch (const std::bad_alloc&) {
        TH_FAIL(TH_ENOMEM, "th_seqset: out of host memory for %lld sets", (long long)n_sets);
    }
    int64_t at_code = 0, at_word = 0, at_pos = 0, at_matrix = 0;
    for (int64_t k = 0; k < n_sets; ++k) {
        const int64_t n = seq_offsets[k + 1] - seq_offsets[k], length = lengths[k];
        if (length < 1) TH_FAIL(TH_EINVAL, "th_seqset: lengths[%lld] = %lld, a set's length is at least 1", (long long)k, (long long)length);
        if (n * length > kMax)
            TH_FAIL(TH_EINVAL, "th_seqset: set %lld has %lld sequences of %lld residues, above 2^31 - 1 in all", (long long)k, (long long)n, (long long)length);
        if (min_matches && (min_matches[k] < 0 || min_matches[k] > length))
            TH_FAIL(TH_EINVAL, "th_seqset: min_matches[%lld] = %d is outside 0 .. lengths[%lld] = %lld", (long long)k, (int)min_matches[k], (long long)k,
                    (long long)length);
        const int64_t words = (length + 3) / 4;
        sets[(size_t)k] = SeqSet{seq_offsets[k], at_code, at_word, at_pos, at_matrix, (int)n, (int)length, (int)words, min_matches ? min_matches[k] : -1};
        pos_offsets[(size_t)k] = at_pos;
        at_code += n * length;
        at_word += n * words;
        at_pos += length;
        at_matrix += n * n;
        if (matrix_out && at_matrix > kMax)
            TH_FAIL(TH_EINVAL, "th_seqset: matrix_out would hold more than 2^31 - 1 entries (the sets up to %lld)", (long long)k);
    }
    pos_offsets[(size_t)n_sets] = at_pos;
    if (at_code != total_codes)
        TH_FAIL(TH_EINVAL, "th_seqset: total_codes = %lld, the sets own %lld residues", (long long)total_codes, (long long)at_code);
    if ((total_codes > 0 && !codes) || (n_seq > 0 && !seq_out) || !profile_out)
        TH_FAIL(TH_EINVAL, "th_seqset: total_codes = %lld needs codes, %lld sequences need seq_out, %lld positions need profile_out",
                (long long)total_codes, (long long)n_seq, (long long)at_pos);
    for (int64_t k = 0; k < total_codes; ++k)
        if (codes[k] > 20) TH_FAIL(TH_EINVAL, "th_seqset: codes[%lld] = %d, a code is at most 20", (long long)k, (int)codes[k]);
    for (int64_t k = 0; native && k < at_pos; ++k)
        if (native[k] > 20) TH_FAIL(TH_EINVAL, "th_seqset: native[%lld] = %d, a code is at most 20", (long long)k, (int)native[k]);
    std::vector<ThTile> rows, columns;
    if (int rc = th_tile_items("th_seqset", "sequences", seq_offsets, n_sets, kRows, rows)) return rc;
    if (int rc = th_tile_items("th_seqset", "positions", pos_offsets.data(), n_sets, kPositions, columns)) return rc;

    const size_t ns = (size_t)n_sets, nq = (size_t)n_seq, np = (size_t)at_pos, nm = matrix_out ? (size_t)at_matrix : 0;
    ThLayout lay;
    const size_t o_codes = lay.take((size_t)total_codes), o_packed = lay.take((size_t)at_word * sizeof(unsigned));
    const size_t o_sets = lay.take(ns * sizeof(SeqSet)), o_rows = lay.take(rows.size() * sizeof(ThTile));
    const size_t o_columns = lay.take(columns.size() * sizeof(ThTile)), o_native = lay.take(native ? np : 0);
    const size_t o_table = lay.take(native ? 400 : 0), o_reps = lay.take(min_matches ? nq * sizeof(int32_t) : 0);
    const size_t o_seq = lay.take(nq * kSeqColumns * sizeof(int32_t)), o_profile = lay.take(np * kCodes * sizeof(int32_t));
    const size_t o_matrix = lay.take(nm * sizeof(int32_t)), o_set = lay.take(ns * 4 * sizeof(int64_t));
    ThCall call;
    if (int rc = call.open("th_seqset", device, lay.bytes, kernel_ms ? 4 : 0)) return rc;
    unsigned char *d_codes = call.at<unsigned char>(o_codes), *d_native = native ? call.at<unsigned char>(o_native) : nullptr;
    signed char* d_table = native ? call.at<signed char>(o_table) : nullptr;
    unsigned* d_packed = call.at<unsigned>(o_packed);
    SeqSet* d_sets = call.at<SeqSet>(o_sets);
    ThTile *d_rows = call.at<ThTile>(o_rows), *d_columns = call.at<ThTile>(o_columns);
    int *d_reps = call.at<int>(o_reps), *d_seq = call.at<int>(o_seq), *d_profile = call.at<int>(o_profile);
    int* d_matrix = matrix_out ? call.at<int>(o_matrix) : nullptr;
    long long* d_set = call.at<long long>(o_set);
    hipStream_t st = call.st[0];
    if (total_codes > 0) HIP_TRY(hipMemcpyAsync(d_codes, codes, (size_t)total_codes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_sets, sets.data(), ns * sizeof(SeqSet), hipMemcpyHostToDevice, st));
    if (!rows.empty()) HIP_TRY(hipMemcpyAsync(d_rows, rows.data(), rows.size() * sizeof(ThTile), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_columns, columns.data(), columns.size() * sizeof(ThTile), hipMemcpyHostToDevice, st));
    if (native) {
        HIP_TRY(hipMemcpyAsync(d_native, native, np, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_table, substitution, 400, hipMemcpyHostToDevice, st));
    }
    const dim3 block(kThreads), row_grid((unsigned)rows.size());
    HIP_TRY(call.mark(0));
    if (!rows.empty()) {
        hipLaunchKernelGGL(k_seqset_pack, row_grid, block, 0, st, d_codes, d_sets, d_rows, d_packed);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_seqset_pairs, row_grid, block, 0, st, d_packed, d_sets, d_rows, d_seq, d_matrix);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_seqset_native, row_grid, block, 0, st, d_codes, d_sets, d_rows, d_native, d_table, d_seq);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_seqset_columns, dim3((unsigned)columns.size()), block, 0, st, d_codes, d_sets, d_columns, d_profile);
    HIP_TRY(hipGetLastError());
    HIP_TRY(call.mark(1));
    hipLaunchKernelGGL(k_seqset_cluster, dim3((unsigned)ns), dim3(kClusterThreads), 0, st, d_packed, d_sets, d_reps, d_seq);
    HIP_TRY(hipGetLastError());
    HIP_TRY(call.mark(2));
    hipLaunchKernelGGL(k_seqset_totals, dim3((unsigned)((ns + kThreads / kWave - 1) / (kThreads / kWave))), block, 0, st, d_sets, (long long)n_sets,
                       d_seq, d_set);
    HIP_TRY(hipGetLastError());
    HIP_TRY(call.mark(3));
    if (nq > 0) HIP_TRY(hipMemcpyAsync(seq_out, d_seq, nq * kSeqColumns * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(profile_out, d_profile, np * kCodes * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (nm > 0) HIP_TRY(hipMemcpyAsync(matrix_out, d_matrix, nm * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(set_out, d_set, ns * 4 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    return call.finish(kernel_ms, 3);
}
