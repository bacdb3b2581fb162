// th_analyse_probs: evaluation of a prediction matrix against the true residues (predict.py --output_analysis) — one streaming
// pass over the [n, k] float16 / float32 probabilities that yields, per row, the predicted residue (the FASTA letter), the rank of
// the true residue and the Shannon entropy in bits, and for the whole matrix the confusion matrix, the rank histogram and three
// counters as 64-bit integers.  The reference spreads the same numbers over design_utils/analyse_utils.py (calculate_metrics,
// calculate_prediction_entropy) and ui.py (BLOSUM62 similarity) and computes them with sklearn / scipy after re-reading the CSV.
//
// Kernel shape: a workgroup of 256 lanes walks tiles of whole rows (<= 24 KB of the matrix each).  A tile is copied into LDS with
// 16-byte loads over its byte range, whatever k and the row alignment are, so the matrix is read once and fully coalesced; the rows
// are then spread over groups of L lanes (L = 4 for k <= 32: sixteen rows per wave; 16 for k <= 128; 64 above: one row per wave),
// every lane strides over the columns of its row, and the group combines its lanes by an xor butterfly in a fixed order — every
// per-row result depends on the row alone (not on the tile, the block or the grid).  Per-row totals go into an LDS histogram; at the
// end each workgroup adds its non-zero bins to the global totals with one 64-bit atomicAdd each.  Integer totals do not depend on the
// order in which workgroups arrive: two calls give the same bytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "common.h"
#include "oneshot.h"

namespace {

constexpr int kAnThreads = 256;
constexpr int kTileBytes = 24576;                         // matrix bytes staged per tile (a 1024-column float32 row is 4 KB)
constexpr int kNumRes = 20;
constexpr int kBinConf = 0, kBinRank = 400, kBinLabelled = 421, kBinNonfinite = 422, kBinSimilar = 423, kBins = 424;
static_assert(sizeof(th_analysis_totals) == kBins * sizeof(int64_t), "th_analysis_totals must be the kernel's bin array");

// BLOSUM62 (Henikoff & Henikoff, PNAS 89:10915, 1992), rows and columns in the residue order ACDEFGHIKLMNPQRSTVWY
const signed char kBlosum62[kNumRes][kNumRes] = {
    { 4,  0, -2, -1, -2,  0, -2, -1, -1, -1, -1, -2, -1, -1, -1,  1,  0,  0, -3, -2},   // A
    { 0,  9, -3, -4, -2, -3, -3, -1, -3, -1, -1, -3, -3, -3, -3, -1, -1, -1, -2, -2},   // C
    {-2, -3,  6,  2, -3, -1, -1, -3, -1, -4, -3,  1, -1,  0, -2,  0, -1, -3, -4, -3},   // D
    {-1, -4,  2,  5, -3, -2,  0, -3,  1, -3, -2,  0, -1,  2,  0,  0, -1, -2, -3, -2},   // E
    {-2, -2, -3, -3,  6, -3, -1,  0, -3,  0,  0, -3, -4, -3, -3, -2, -2, -1,  1,  3},   // F
    { 0, -3, -1, -2, -3,  6, -2, -4, -2, -4, -3,  0, -2, -2, -2,  0, -2, -3, -2, -3},   // G
    {-2, -3, -1,  0, -1, -2,  8, -3, -1, -3, -2,  1, -2,  0,  0, -1, -2, -3, -2,  2},   // H
    {-1, -1, -3, -3,  0, -4, -3,  4, -3,  2,  1, -3, -3, -3, -3, -2, -1,  3, -3, -1},   // I
    {-1, -3, -1,  1, -3, -2, -1, -3,  5, -2, -1,  0, -1,  1,  2,  0, -1, -2, -3, -2},   // K
    {-1, -1, -4, -3,  0, -4, -3,  2, -2,  4,  2, -3, -3, -2, -2, -2, -1,  1, -2, -1},   // L
    {-1, -1, -3, -2,  0, -3, -2,  1, -1,  2,  5, -2, -2,  0, -1, -1, -1,  1, -1, -1},   // M
    {-2, -3,  1,  0, -3,  0,  1, -3,  0, -3, -2,  6, -2,  0,  0,  1,  0, -3, -4, -2},   // N
    {-1, -3, -1, -1, -4, -2, -2, -3, -1, -3, -2, -2,  7, -1, -2, -1, -1, -2, -4, -3},   // P
    {-1, -3,  0,  2, -3, -2,  0, -3,  1, -2,  0,  0, -1,  5,  1,  0, -1, -2, -2, -1},   // Q
    {-1, -3, -2,  0, -3, -2,  0, -3,  2, -2, -1,  0, -2,  1,  5, -1, -1, -3, -3, -2},   // R
    { 1, -1,  0,  0, -2,  0, -1, -2,  0, -2, -1,  1, -1,  0, -1,  4,  1, -2, -3, -2},   // S
    { 0, -1, -1, -1, -2, -2, -2, -1, -1, -1, -1,  0, -1, -1, -1,  1,  5,  0, -2, -2},   // T
    { 0, -1, -3, -2, -1, -3, -3,  3, -2,  1,  1, -3, -2, -2, -3, -2,  0,  4, -3, -1},   // V
    {-3, -2, -4, -3,  1, -2, -2, -3, -3, -2, -1, -4, -4, -2, -3, -3, -2, -3, 11,  2},   // W
    {-2, -2, -3, -2,  3, -3,  2, -1, -2, -1, -1, -2, -3, -1, -2, -2, -2, -1,  2,  7},   // Y
};

struct AnArgs {
    const void* x;                 // [n, k] rows of this block (16-byte aligned device memory, readable up to the next 16 bytes)
    const int8_t* true_res;        // [n]
    const int8_t* col_res;         // [k]
    int8_t* pred;                  // [n] or null
    int8_t* rank;                  // [n] or null
    double* ent;                   // [n] or null
    unsigned long long* totals;    // [kBins]
    long long n;
    int k;
    uint32_t similar[kNumRes];     // bit p of similar[t]: BLOSUM62(t, p) > 0
};

template <bool F16>
__device__ __forceinline__ float an_load(const unsigned char* row, int c) {
    if constexpr (F16) return (float)__builtin_bit_cast(_Float16, ((const uint16_t*)row)[c]);
    else return ((const float*)row)[c];
}

// p * log2(p) for a finite p > 0, in float64.  float16: p = 2^(e-15) (1 + m/1024) or, subnormal, m 2^-24 — the logarithm is the
// exponent plus a table entry (lg[m] = log2(1 + m/1024), lg[1024 + m] = log2(m)), exact up to the two roundings of the sum and the
// product; float32: the float64 log2 of the value.
template <bool F16>
__device__ __forceinline__ double an_plog(const unsigned char* row, int c, float v, const double* lg) {
    if constexpr (F16) {
        const uint32_t h = ((const uint16_t*)row)[c];
        const int e = (int)((h >> 10) & 31), m = (int)(h & 1023);
        const double l = e ? (double)(e - 15) + lg[m] : lg[1024 + m] - 24.0;
        return (double)v * l;
    } else {
        return (double)v * log2((double)v);
    }
}

// "other beats mine" under np.argmax's rules: the first NaN wins, then the larger value, then the lower column
__device__ __forceinline__ bool an_argmax_takes(float ov, int oc, float mv, int mc) {
    if (oc < 0) return false;
    if (mc < 0) return true;
    const bool on = ov != ov, mn = mv != mv;
    if (on != mn) return on;
    if (on || ov == mv) return oc < mc;
    return ov > mv;
}

template <bool F16, int L>
__global__ void __launch_bounds__(kAnThreads) k_analyse(AnArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char tile[kTileBytes + 32];
    __shared__ double lg[F16 ? 2048 : 1];
    __shared__ int8_t cres[1024];
    __shared__ unsigned int hist[kBins];
    constexpr int esz = F16 ? 2 : 4, G = kAnThreads / L;
    const int tid = threadIdx.x, lane = tid & (L - 1), grp = tid / L, k = a.k;
    for (int i = tid; i < kBins; i += kAnThreads) hist[i] = 0;
    for (int i = tid; i < k; i += kAnThreads) cres[i] = a.col_res[i];
    if constexpr (F16) {
        for (int i = tid; i < 1024; i += kAnThreads) {
            lg[i] = log2(1.0 + (double)i / 1024.0);
            lg[1024 + i] = i ? log2((double)i) : 0.0;
        }
    }
    const long long rows_per_tile = std::max(1, kTileBytes / (k * esz));
    const long long n_tiles = (a.n + rows_per_tile - 1) / rows_per_tile;
    for (long long ti = blockIdx.x; ti < n_tiles; ti += gridDim.x) {
        const long long r0 = ti * rows_per_tile, r1 = std::min(a.n, r0 + rows_per_tile);
        const long long b0 = r0 * k * esz, b1 = r1 * k * esz, a0 = b0 & ~15LL;
        const int nw = (int)((b1 - a0 + 15) >> 4);
        const uint4* src = (const uint4*)((const unsigned char*)a.x + a0);
        __syncthreads();                                       // the previous tile is no longer read (and the tables are in place)
        for (int w = tid; w < nw; w += kAnThreads) ((uint4*)tile)[w] = src[w];
        __syncthreads();
        const unsigned char* base = tile + (b0 - a0);
        for (long long r = r0 + grp; r < r1; r += G) {
            const unsigned char* row = base + (size_t)(r - r0) * k * esz;
            const int t = a.true_res[r];
            // pass 1: arg-max, the true residue's score (max over its columns, first column reaching it), sums for the entropy
            float bv = 0.f, sv = 0.f;
            int bc = -1, sc = -1;
            bool bad = false, neg = false;
            double S = 0.0, P = 0.0;
            for (int c = lane; c < k; c += L) {
                const float v = an_load<F16>(row, c);
                bad |= !(fabsf(v) <= 3.402823466e38f);         // NaN or infinite
                neg |= v < 0.f;
                if (an_argmax_takes(v, c, bv, bc)) { bv = v; bc = c; }
                if (cres[c] == t && (sc < 0 || v > sv)) { sv = v; sc = c; }
                S += (double)v;
                if (v > 0.f) P += an_plog<F16>(row, c, v, lg);
            }
#pragma unroll
            for (int m = L / 2; m >= 1; m >>= 1) {
                const float obv = __shfl_xor(bv, m, L), osv = __shfl_xor(sv, m, L);
                const int obc = __shfl_xor(bc, m, L), osc = __shfl_xor(sc, m, L);
                if (an_argmax_takes(obv, obc, bv, bc)) { bv = obv; bc = obc; }
                if (osc >= 0 && (sc < 0 || osv > sv || (osv == sv && osc < sc))) { sv = osv; sc = osc; }
                bad |= __shfl_xor((int)bad, m, L) != 0;
                neg |= __shfl_xor((int)neg, m, L) != 0;
                S += __shfl_xor(S, m, L);
                P += __shfl_xor(P, m, L);
            }
            const int pred = cres[bc];
            // pass 2: the residues with a column that beats the true residue's (score, first column)
            int rank = -1;
            if (t >= 0) {
                if (bad) rank = pred == t ? 0 : kNumRes;
                else if (sc < 0) rank = kNumRes;
                else {
                    uint32_t mask = 0;
                    for (int c = lane; c < k; c += L) {
                        const int rc = cres[c];
                        if (rc == t) continue;
                        const float v = an_load<F16>(row, c);
                        if (v > sv || (v == sv && c < sc)) mask |= 1u << rc;
                    }
#pragma unroll
                    for (int m = L / 2; m >= 1; m >>= 1) mask |= (uint32_t)__shfl_xor((int)mask, m, L);
                    rank = __popc(mask);
                }
            }
            if (lane == 0) {
                if (a.pred) a.pred[r] = (int8_t)pred;
                if (a.rank) a.rank[r] = (int8_t)rank;
                if (a.ent) a.ent[r] = (bad || neg || !(S > 0.0)) ? __builtin_nan("") : log2(S) - P / S;
                if (t >= 0) {
                    atomicAdd(&hist[kBinConf + t * kNumRes + pred], 1u);
                    atomicAdd(&hist[kBinRank + rank], 1u);
                    atomicAdd(&hist[kBinLabelled], 1u);
                    if ((a.similar[t] >> pred) & 1u) atomicAdd(&hist[kBinSimilar], 1u);
                }
                if (bad) atomicAdd(&hist[kBinNonfinite], 1u);
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < kBins; i += kAnThreads)
        if (hist[i]) atomicAdd(&a.totals[i], (unsigned long long)hist[i]);
}

template <bool F16>
void an_launch(hipStream_t s, int blocks, const AnArgs& a) {
    if (a.k <= 32) hipLaunchKernelGGL((k_analyse<F16, 4>), dim3(blocks), dim3(kAnThreads), 0, s, a);
    else if (a.k <= 128) hipLaunchKernelGGL((k_analyse<F16, 16>), dim3(blocks), dim3(kAnThreads), 0, s, a);
    else hipLaunchKernelGGL((k_analyse<F16, 64>), dim3(blocks), dim3(kAnThreads), 0, s, a);
}

}  // namespace

// rows staged per block by th_analyse_probs and th_analyse_classes: a few hundred thousand, at most 256 MB of matrix.
// TH_ANALYSIS_BLOCK_ROWS overrides it (tests: the blocking must not change a single result)
int64_t th_analysis_block_rows(size_t row_bytes, int64_t n) {
    int64_t block = std::min<int64_t>(262144, std::max<int64_t>(1, (int64_t)((256u << 20) / row_bytes)));
    if (const char* e = std::getenv("TH_ANALYSIS_BLOCK_ROWS")) {
        const long long v = std::atoll(e);
        if (v > 0) block = v;
    }
    return std::min<int64_t>(block, n);
}

extern "C" int th_analyse_probs(int device, const void* matrix, int dtype, int64_t n, int64_t k, const int8_t* col_res,
                                const int8_t* true_res, int8_t* pred_out, int8_t* rank_out, double* entropy_out,
                                th_analysis_totals* totals) {
    if (!totals || !col_res || n < 0 || (n > 0 && (!matrix || !true_res))) TH_FAIL(TH_EINVAL, "th_analyse_probs: bad argument");
    if (dtype != TH_F16 && dtype != TH_F32) TH_FAIL(TH_EINVAL, "th_analyse_probs: dtype must be f16 or f32");
    if (k < 1 || k > 1024) TH_FAIL(TH_EINVAL, "th_analyse_probs: k = %lld outside 1..1024", (long long)k);
    for (int64_t c = 0; c < k; ++c)
        if (col_res[c] < 0 || col_res[c] >= kNumRes) TH_FAIL(TH_EINVAL, "th_analyse_probs: col_res[%lld] = %d outside 0..19", (long long)c, (int)col_res[c]);
    for (int64_t i = 0; i < n; ++i)
        if (true_res[i] < -1 || true_res[i] >= kNumRes) TH_FAIL(TH_EINVAL, "th_analyse_probs: true_res[%lld] = %d outside -1..19", (long long)i, (int)true_res[i]);
    std::memset(totals, 0, sizeof(*totals));
    if (n == 0) return TH_OK;

    const size_t esz = dtype == TH_F16 ? 2 : 4, row_bytes = esz * (size_t)k;
    const int64_t block = th_analysis_block_rows(row_bytes, n);
    const int64_t n_blocks = (n + block - 1) / block;
    const int slots = n_blocks > 1 ? 2 : 1;

    ThCall call;
    HIP_TRY(hipSetDevice(device));
    call.device = device;
    int ncu = 0;
    HIP_TRY(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device));
    // one allocation: totals, col_res, then per slot the matrix block (+16 bytes: the tile loads round the last row up to 16),
    // true residues and the per-row outputs
    ThLayout lay, slot_lay;
    const size_t o_tot = lay.take(kBins * sizeof(unsigned long long)), o_cres = lay.take((size_t)k), off_slot = lay.bytes;
    const size_t o_x = slot_lay.take(block * row_bytes + 16), o_true = slot_lay.take((size_t)block), o_pred = slot_lay.take((size_t)block);
    const size_t o_rank = slot_lay.take((size_t)block), o_ent = slot_lay.take((size_t)block * sizeof(double)), slot_bytes = slot_lay.bytes;
    if (int rc = th_alloc_or_fail("th_analyse_probs", &call.mem[0], off_slot + slots * slot_bytes)) return rc;
    for (int s = 0; s < slots; ++s) HIP_TRY(hipStreamCreateWithFlags(&call.st[s], hipStreamNonBlocking));
    unsigned long long* d_tot = call.at<unsigned long long>(o_tot);
    int8_t* d_cres = call.at<int8_t>(o_cres);
    HIP_TRY(hipMemsetAsync(d_tot, 0, kBins * sizeof(unsigned long long), call.st[0]));
    HIP_TRY(hipMemcpyAsync(d_cres, col_res, (size_t)k, hipMemcpyHostToDevice, call.st[0]));
    HIP_TRY(hipStreamSynchronize(call.st[0]));          // both streams' kernels add into d_tot

    AnArgs a{};
    a.col_res = d_cres;
    a.totals = d_tot;
    a.k = (int)k;
    for (int t = 0; t < kNumRes; ++t)
        for (int p = 0; p < kNumRes; ++p)
            if (kBlosum62[t][p] > 0) a.similar[t] |= 1u << p;
    // block b runs on stream b % 2 in slot b % 2: the copy of block b + 1 overlaps the kernel of block b, and a slot is only
    // overwritten after the stream has finished with it
    for (int64_t b = 0; b < n_blocks; ++b) {
        const int s = (int)(b % slots);
        hipStream_t st = call.st[s];
        unsigned char* slot = call.at<unsigned char>(off_slot + s * slot_bytes + o_x);
        const int64_t lo = b * block, rows = std::min(block, n - lo);
        int8_t *d_true = (int8_t*)(slot + o_true), *d_pred = (int8_t*)(slot + o_pred), *d_rank = (int8_t*)(slot + o_rank);
        double* d_ent = (double*)(slot + o_ent);
        HIP_TRY(hipMemcpyAsync(slot, (const unsigned char*)matrix + lo * row_bytes, rows * row_bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_true, true_res + lo, (size_t)rows, hipMemcpyHostToDevice, st));
        a.x = slot;
        a.true_res = d_true;
        a.pred = pred_out ? d_pred : nullptr;
        a.rank = rank_out ? d_rank : nullptr;
        a.ent = entropy_out ? d_ent : nullptr;
        a.n = rows;
        const int64_t rows_per_tile = std::max<int64_t>(1, kTileBytes / (int64_t)row_bytes);
        const int blocks = (int)std::min<int64_t>((rows + rows_per_tile - 1) / rows_per_tile, (int64_t)std::max(ncu, 1) * 3);
        if (dtype == TH_F16) an_launch<true>(st, blocks, a);
        else an_launch<false>(st, blocks, a);
        HIP_TRY(hipGetLastError());
        if (pred_out) HIP_TRY(hipMemcpyAsync(pred_out + lo, d_pred, (size_t)rows, hipMemcpyDeviceToHost, st));
        if (rank_out) HIP_TRY(hipMemcpyAsync(rank_out + lo, d_rank, (size_t)rows, hipMemcpyDeviceToHost, st));
        if (entropy_out) HIP_TRY(hipMemcpyAsync(entropy_out + lo, d_ent, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    for (int s = 1; s < slots; ++s) HIP_TRY(hipStreamSynchronize(call.st[s]));
    HIP_TRY(hipMemcpyAsync(totals, d_tot, sizeof(*totals), hipMemcpyDeviceToHost, call.st[0]));
    HIP_TRY(hipStreamSynchronize(call.st[0]));
    return TH_OK;
}
