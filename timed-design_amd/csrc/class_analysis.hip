// th_analyse_classes: per-CLASS evaluation of a prediction matrix (analyse_rotamers.py, predict.py --output_auc) — for a [n, k]
// float16 / float32 matrix and one true class per row: the predicted class and the rank of the true class per row, the k x k
// confusion matrix, the rank histogram, the number of scored rows per class and, for the ROC AUC one-vs-one and one-vs-rest, the
// table U2[a][b] = twice the Mann-Whitney statistic of column a, class-a rows against class-b rows (ties count half).  The reference
// computes these with sklearn (design_utils/analyse_utils.py calculate_rotamer_metrics); its OvO AUC loops over k (k - 1) / 2 class
// pairs with masks over all n rows.  Everything here is a 64-bit integer: two calls give the same bytes, whatever the grid, the
// staging blocks or the order in which workgroups arrive.
//
// Three steps, the matrix staged from the host in the same row blocks as th_analyse_probs (two slots, two streams):
//   1. k_class_rows (streaming, the shape of k_analyse: tiles of whole rows into LDS with 16-byte loads, a lane group per row):
//      arg-max, rank of the true class, finite flag, and the row's own-class score x[i][y_i] as an order-preserving 32-bit key
//      (-0 folded onto +0) packed as (class << 32 | key); a row that is not scored packs to all ones.  Rank histogram, counters and
//      per-class counts go through an LDS histogram; the k x k confusion matrix does so for k <= 32, above that it does not fit
//      LDS (338^2 x 4 B = 457 KB) and takes one 64-bit global atomicAdd per labelled row.
//   2. the n packed values are sorted once on the device (rocPRIM radix sort, 43 bits): the scored rows come out grouped by class
//      and sorted by key within the class, the others at the end.  The low halves become the "positives" table (4 bytes per scored
//      row, 4 MB for a million rows: resident in L2 / Infinity Cache), the class offsets are the prefix sums of scored_count.
//   3. k_pair_sweep, the hot path: a second pass over the matrix.  When the whole matrix is one staging block it is still
//      resident from step 1 and is not copied again; otherwise the blocks are re-staged from the host.  The host groups the
//      labelled rows of each block by true class (a counting sort over int16 labels, no matrix access) and cuts every class
//      into runs of up to 64 rows; a workgroup takes one run of class b.  A thread owns a column a (and a + 256, ... for k > 256;
//      for k < 256 the 256 lanes form 256 / k row lanes), loads x[row][a] for the rows of the run — contiguous across the
//      workgroup — and finds with a binary search among class a's sorted positives how many are greater and how many equal:
//      2 * greater + equal = 2 n_a - lower_bound - upper_bound accumulates in a 64-bit register, is combined across row lanes in
//      LDS, and ends in one global atomicAdd per (a, b) and run.  Column a = b and rows that are not scored are skipped.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "common.h"
#include "oneshot.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTileBytes = 24576;             // matrix bytes staged per tile of the row pass
constexpr int kMaxK = 1024;
constexpr int kConfLds = 32;                  // k up to which the row pass keeps the confusion matrix in its LDS histogram
constexpr int kRun = 64;                      // rows of one class per workgroup of the sweep
constexpr unsigned long long kNotScored = ~0ull;
constexpr unsigned kSortBits = 43;            // 32 key bits + 10 class bits + bit 42, which only kNotScored sets

struct Run { int cls, start, count; };        // rows order[start .. start + count) of a block, all of true class cls

template <bool F16>
__device__ __forceinline__ float cl_load(const void* x, long long i) {
    if constexpr (F16) return (float)__builtin_bit_cast(_Float16, ((const uint16_t*)x)[i]);
    else return ((const float*)x)[i];
}

// order-preserving key of a finite value: a < b <=> key(a) < key(b), key(-0) == key(+0)
__device__ __forceinline__ uint32_t cl_key(float v) {
    const uint32_t u = v == 0.f ? 0u : __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// "other beats mine" under np.argmax's rules: the first NaN wins, then the larger value, then the lower column
__device__ __forceinline__ bool cl_argmax_takes(float ov, int oc, float mv, int mc) {
    if (oc < 0) return false;
    if (mc < 0) return true;
    const bool on = ov != ov, mn = mv != mv;
    if (on != mn) return on;
    if (on || ov == mv) return oc < mc;
    return ov > mv;
}

struct RowArgs {
    const void* x;                     // [n, k] rows of this block (16-byte aligned, readable up to the next 16 bytes)
    const int16_t* true_class;         // [n]
    int16_t* pred;                     // [n] or null
    int16_t* rank;                     // [n] or null
    unsigned long long* packed;        // [n] or null (no AUC sweep)
    unsigned char* scored;             // [n] or null
    unsigned long long* confusion;     // [k * k]
    unsigned long long* rank_hist;     // [k + 1]
    unsigned long long* scored_count;  // [k]
    unsigned long long* counts;        // n_labelled, n_nonfinite, n_scored
    long long n;
    int k;
};

template <bool F16, int L>
__global__ void __launch_bounds__(kThreads) k_class_rows(RowArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char tile[kTileBytes + 32];
    __shared__ unsigned int h_rank[kMaxK + 1], h_scored[kMaxK], h_counts[3];
    __shared__ unsigned int h_conf[kConfLds * kConfLds];      // the confusion matrix of a small k (20 residues) fits LDS too
    constexpr int esz = F16 ? 2 : 4, G = kThreads / L;
    const int tid = threadIdx.x, lane = tid & (L - 1), grp = tid / L, k = a.k;
    for (int i = tid; i <= k; i += kThreads) h_rank[i] = 0;
    for (int i = tid; i < k; i += kThreads) h_scored[i] = 0;
    if (tid < 3) h_counts[tid] = 0;
    const bool conf_lds = k <= kConfLds;
    if (conf_lds)
        for (int i = tid; i < k * k; i += kThreads) h_conf[i] = 0;
    const long long rows_per_tile = std::max(1, kTileBytes / (k * esz));
    const long long n_tiles = (a.n + rows_per_tile - 1) / rows_per_tile;
    for (long long ti = blockIdx.x; ti < n_tiles; ti += gridDim.x) {
        const long long r0 = ti * rows_per_tile, r1 = std::min(a.n, r0 + rows_per_tile);
        const long long b0 = r0 * k * esz, b1 = r1 * k * esz, a0 = b0 & ~15LL;
        const int nw = (int)((b1 - a0 + 15) >> 4);
        const uint4* src = (const uint4*)((const unsigned char*)a.x + a0);
        __syncthreads();                                       // the previous tile is no longer read (and the histograms are zero)
        for (int w = tid; w < nw; w += kThreads) ((uint4*)tile)[w] = src[w];
        __syncthreads();
        const unsigned char* base = tile + (b0 - a0);
        for (long long r = r0 + grp; r < r1; r += G) {
            const unsigned char* row = base + (size_t)(r - r0) * k * esz;
            const int t = a.true_class[r];
            const float tv = t >= 0 ? cl_load<F16>(row, t) : 0.f;
            float bv = 0.f;
            int bc = -1, above = 0;
            bool bad = false;
            for (int c = lane; c < k; c += L) {
                const float v = cl_load<F16>(row, c);
                bad |= !(fabsf(v) <= 3.402823466e38f);         // NaN or infinite
                if (cl_argmax_takes(v, c, bv, bc)) { bv = v; bc = c; }
                above += (v > tv || (v == tv && c < t)) ? 1 : 0;
            }
#pragma unroll
            for (int m = L / 2; m >= 1; m >>= 1) {
                const float obv = __shfl_xor(bv, m, L);
                const int obc = __shfl_xor(bc, m, L);
                if (cl_argmax_takes(obv, obc, bv, bc)) { bv = obv; bc = obc; }
                bad |= __shfl_xor((int)bad, m, L) != 0;
                above += __shfl_xor(above, m, L);
            }
            if (lane == 0) {
                const int rank = t < 0 ? -1 : bad ? (bc == t ? 0 : k) : above;
                if (a.pred) a.pred[r] = (int16_t)bc;
                if (a.rank) a.rank[r] = (int16_t)rank;
                const bool scored = t >= 0 && !bad;
                if (a.packed) a.packed[r] = scored ? ((unsigned long long)t << 32) | cl_key(tv) : kNotScored;
                if (a.scored) a.scored[r] = scored ? 1 : 0;
                if (t >= 0) {
                    if (conf_lds) atomicAdd(&h_conf[t * k + bc], 1u);
                    else atomicAdd(&a.confusion[(size_t)t * k + bc], 1ull);
                    atomicAdd(&h_rank[rank], 1u);
                    atomicAdd(&h_counts[0], 1u);
                }
                if (bad) atomicAdd(&h_counts[1], 1u);
                if (scored) {
                    atomicAdd(&h_counts[2], 1u);
                    atomicAdd(&h_scored[t], 1u);
                }
            }
        }
    }
    __syncthreads();
    for (int i = tid; i <= k; i += kThreads)
        if (h_rank[i]) atomicAdd(&a.rank_hist[i], (unsigned long long)h_rank[i]);
    for (int i = tid; i < k; i += kThreads)
        if (h_scored[i]) atomicAdd(&a.scored_count[i], (unsigned long long)h_scored[i]);
    if (tid < 3 && h_counts[tid]) atomicAdd(&a.counts[tid], (unsigned long long)h_counts[tid]);
    if (conf_lds)
        for (int i = tid; i < k * k; i += kThreads)
            if (h_conf[i]) atomicAdd(&a.confusion[i], (unsigned long long)h_conf[i]);
}

template <bool F16>
void rows_launch(hipStream_t s, int blocks, const RowArgs& a) {
    if (a.k <= 32) hipLaunchKernelGGL((k_class_rows<F16, 4>), dim3(blocks), dim3(kThreads), 0, s, a);
    else if (a.k <= 128) hipLaunchKernelGGL((k_class_rows<F16, 16>), dim3(blocks), dim3(kThreads), 0, s, a);
    else hipLaunchKernelGGL((k_class_rows<F16, 64>), dim3(blocks), dim3(kThreads), 0, s, a);
}

// the positives table: the key halves of the first n_scored sorted values
__global__ void __launch_bounds__(kThreads) k_positives(const unsigned long long* sorted, uint32_t* keys, long long n_scored) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i < n_scored) keys[i] = (uint32_t)sorted[i];
}

struct SweepArgs {
    const void* x;                     // [rows, k] of this block
    const unsigned char* scored;       // [rows]
    const int* order;                  // row indices of this block grouped by class
    const Run* runs;                   // one per workgroup
    const uint32_t* keys;              // [n_scored] positives, sorted within each class
    const long long* offset;           // [k + 1] class offsets into keys
    unsigned long long* u2;            // [k * k]
    int k;
};

template <bool F16>
__global__ void __launch_bounds__(kThreads) k_pair_sweep(SweepArgs a) {
    __shared__ unsigned long long acc[kMaxK];
    __shared__ int rows[kRun];
    const int tid = threadIdx.x, k = a.k;
    const Run run = a.runs[blockIdx.x];
    for (int i = tid; i < k; i += kThreads) acc[i] = 0;
    if (tid < run.count) {
        const int r = a.order[run.start + tid];
        rows[tid] = a.scored[r] ? r : -1;
    }
    __syncthreads();
    const int kc = k < kThreads ? k : kThreads, row_lanes = kThreads / kc;
    const int col0 = tid % kc, rl = tid / kc;
    if (rl < row_lanes) {
        for (int c = col0; c < k; c += kThreads) {
            if (c == run.cls) continue;
            const long long o = a.offset[c];
            const uint32_t na = (uint32_t)(a.offset[c + 1] - o);
            if (!na) continue;
            const uint32_t* tab = a.keys + o;
            unsigned long long sum = 0;
            for (int j = rl; j < run.count; j += row_lanes) {
                const int r = rows[j];
                if (r < 0) continue;
                const uint32_t key = cl_key(cl_load<F16>(a.x, (long long)r * k + c));
                uint32_t lo = 0, hi = na;                      // lower bound: positives below the key
                while (lo < hi) {
                    const uint32_t mid = lo + ((hi - lo) >> 1);
                    if (tab[mid] < key) lo = mid + 1;
                    else hi = mid;
                }
                uint32_t ub = lo;
                if (lo < na && tab[lo] == key) {               // ties: upper bound among the rest
                    uint32_t l2 = lo + 1, h2 = na;
                    while (l2 < h2) {
                        const uint32_t mid = l2 + ((h2 - l2) >> 1);
                        if (tab[mid] <= key) l2 = mid + 1;
                        else h2 = mid;
                    }
                    ub = l2;
                }
                sum += 2ull * na - lo - ub;                    // 2 * greater + equal
            }
            if (sum) atomicAdd(&acc[c], sum);
        }
    }
    __syncthreads();
    for (int c = tid; c < k; c += kThreads)
        if (acc[c]) atomicAdd(&a.u2[(size_t)c * k + run.cls], acc[c]);
}

// labelled rows of every staging block grouped by true class, cut into runs of at most kRun rows
struct Grouping {
    std::vector<int> order;            // [labelled rows], block after block
    std::vector<Run> runs;
    std::vector<size_t> order_lo, run_lo;      // [n_blocks + 1]
};

void group_rows(const int16_t* true_class, int64_t n, int64_t k, int64_t block, Grouping& g) {
    const int64_t n_blocks = (n + block - 1) / block;
    std::vector<int> start((size_t)k + 1);
    g.order_lo.assign(1, 0);
    g.run_lo.assign(1, 0);
    for (int64_t b = 0; b < n_blocks; ++b) {
        const int64_t lo = b * block, rows = std::min(block, n - lo);
        std::fill(start.begin(), start.end(), 0);
        for (int64_t i = 0; i < rows; ++i)
            if (true_class[lo + i] >= 0) ++start[true_class[lo + i] + 1];
        for (int64_t c = 0; c < k; ++c) start[c + 1] += start[c];
        const size_t base = g.order.size();
        g.order.resize(base + (size_t)start[k]);
        for (int64_t c = 0; c < k; ++c)
            for (int s = start[c]; s < start[c + 1]; s += kRun) g.runs.push_back(Run{(int)c, s, std::min(kRun, start[c + 1] - s)});
        for (int64_t i = 0; i < rows; ++i)
            if (true_class[lo + i] >= 0) g.order[base + (size_t)start[true_class[lo + i]]++] = (int)i;
        g.order_lo.push_back(g.order.size());
        g.run_lo.push_back(g.runs.size());
    }
}

}  // namespace

extern "C" int th_analyse_classes(int device, const void* matrix, int dtype, int64_t n, int64_t k, const int16_t* true_class,
                                  int16_t* pred_out, int16_t* rank_out, int64_t* confusion, int64_t* rank_hist,
                                  int64_t* scored_count, int64_t* pair_u2, th_class_counts* counts) {
    if (!confusion || !rank_hist || !scored_count || !counts || n < 0 || (n > 0 && (!matrix || !true_class)))
        TH_FAIL(TH_EINVAL, "th_analyse_classes: bad argument");
    if (dtype != TH_F16 && dtype != TH_F32) TH_FAIL(TH_EINVAL, "th_analyse_classes: dtype must be f16 or f32");
    if (k < 1 || k > kMaxK) TH_FAIL(TH_EINVAL, "th_analyse_classes: k = %lld outside 1..1024", (long long)k);
    if (n > INT_MAX) TH_FAIL(TH_EINVAL, "th_analyse_classes: n = %lld above 2^31 - 1", (long long)n);
    for (int64_t i = 0; i < n; ++i)
        if (true_class[i] < -1 || true_class[i] >= k)
            TH_FAIL(TH_EINVAL, "th_analyse_classes: true_class[%lld] = %d outside -1..%lld", (long long)i, (int)true_class[i], (long long)k - 1);
    const size_t kk = (size_t)k * (size_t)k;
    std::memset(confusion, 0, kk * sizeof(int64_t));
    std::memset(rank_hist, 0, ((size_t)k + 1) * sizeof(int64_t));
    std::memset(scored_count, 0, (size_t)k * sizeof(int64_t));
    if (pair_u2) std::memset(pair_u2, 0, kk * sizeof(int64_t));
    std::memset(counts, 0, sizeof(*counts));
    if (n == 0) return TH_OK;

    const size_t esz = dtype == TH_F16 ? 2 : 4, row_bytes = esz * (size_t)k;
    const int64_t block = th_analysis_block_rows(row_bytes, n);       // as th_analyse_probs
    const int64_t n_blocks = (n + block - 1) / block;
    const int slots = n_blocks > 1 ? 2 : 1;
    const bool auc = pair_u2 != nullptr;

    Grouping grp;
    std::vector<long long> offset((size_t)k + 1, 0);
    if (auc) {
        try {
            group_rows(true_class, n, k, block, grp);
        } catch (const std::bad_alloc&) {
            TH_FAIL(TH_ENOMEM, "th_analyse_classes: out of host memory grouping %lld rows", (long long)n);
        }
    }
    size_t max_order = 0, max_runs = 0;
    for (int64_t b = 0; auc && b < n_blocks; ++b) {
        max_order = std::max(max_order, grp.order_lo[b + 1] - grp.order_lo[b]);
        max_runs = std::max(max_runs, grp.run_lo[b + 1] - grp.run_lo[b]);
    }

    ThCall call;
    HIP_TRY(hipSetDevice(device));
    call.device = device;
    int ncu = 0;
    HIP_TRY(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device));
    // one allocation: the totals (confusion, rank_hist, scored_count, counts, u2), the class offsets, per row of the whole matrix
    // the packed value (twice: the sort's output), the positives and the scored flag, then per slot the matrix block (+16 bytes:
    // the tile loads round the last row up to 16), its labels, per-row outputs, row order and runs
    const size_t n_tot = kk + ((size_t)k + 1) + (size_t)k + 3 + (auc ? kk : 0);
    ThLayout lay, slot_lay;
    const size_t o_tot = lay.take(n_tot * sizeof(unsigned long long)), o_offset = lay.take(((size_t)k + 1) * sizeof(long long));
    const size_t o_packed = lay.take(auc ? (size_t)n * 8 : 0), o_sorted = lay.take(auc ? (size_t)n * 8 : 0);
    const size_t o_keys = lay.take(auc ? (size_t)n * 4 : 0), o_flag = lay.take(auc ? (size_t)n : 0), off_slot = lay.bytes;
    const size_t o_x = slot_lay.take(block * row_bytes + 16), o_true = slot_lay.take((size_t)block * 2), o_pred = slot_lay.take((size_t)block * 2);
    const size_t o_rank = slot_lay.take((size_t)block * 2), o_order = slot_lay.take(max_order * sizeof(int)), o_runs = slot_lay.take(max_runs * sizeof(Run));
    const size_t slot_bytes = slot_lay.bytes;
    if (int rc = th_alloc_or_fail("th_analyse_classes", &call.mem[0], off_slot + slots * slot_bytes)) return rc;
    for (int s = 0; s < slots; ++s) HIP_TRY(hipStreamCreateWithFlags(&call.st[s], hipStreamNonBlocking));
    unsigned long long* d_conf = call.at<unsigned long long>(o_tot);
    unsigned long long* d_rank_hist = d_conf + kk;
    unsigned long long* d_scored_count = d_rank_hist + k + 1;
    unsigned long long* d_counts = d_scored_count + k;
    unsigned long long* d_u2 = d_counts + 3;
    long long* d_offset = call.at<long long>(o_offset);
    unsigned long long *d_packed = call.at<unsigned long long>(o_packed), *d_sorted = call.at<unsigned long long>(o_sorted);
    uint32_t* d_keys = call.at<uint32_t>(o_keys);
    unsigned char* d_flag = call.at<unsigned char>(o_flag);
    HIP_TRY(hipMemsetAsync(d_conf, 0, n_tot * sizeof(unsigned long long), call.st[0]));
    HIP_TRY(hipStreamSynchronize(call.st[0]));          // both streams' kernels add into the totals

    auto slot_of = [&](int s) { return call.at<unsigned char>(off_slot + s * slot_bytes + o_x); };
    // ---- step 1: the row pass.  Block b runs on stream b % 2 in slot b % 2: the copy of block b + 1 overlaps the kernel of block b
    RowArgs ra{};
    ra.confusion = d_conf;
    ra.rank_hist = d_rank_hist;
    ra.scored_count = d_scored_count;
    ra.counts = d_counts;
    ra.k = (int)k;
    for (int64_t b = 0; b < n_blocks; ++b) {
        const int s = (int)(b % slots);
        hipStream_t st = call.st[s];
        unsigned char* slot = slot_of(s);
        const int64_t lo = b * block, rows = std::min(block, n - lo);
        int16_t *d_true = (int16_t*)(slot + o_true), *d_pred = (int16_t*)(slot + o_pred), *d_rank = (int16_t*)(slot + o_rank);
        HIP_TRY(hipMemcpyAsync(slot, (const unsigned char*)matrix + lo * row_bytes, rows * row_bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_true, true_class + lo, (size_t)rows * 2, hipMemcpyHostToDevice, st));
        ra.x = slot;
        ra.true_class = d_true;
        ra.pred = pred_out ? d_pred : nullptr;
        ra.rank = rank_out ? d_rank : nullptr;
        ra.packed = auc ? d_packed + lo : nullptr;
        ra.scored = auc ? d_flag + lo : nullptr;
        ra.n = rows;
        const int64_t rows_per_tile = std::max<int64_t>(1, kTileBytes / (int64_t)row_bytes);
        const int blocks = (int)std::min<int64_t>((rows + rows_per_tile - 1) / rows_per_tile, (int64_t)std::max(ncu, 1) * 3);
        if (dtype == TH_F16) rows_launch<true>(st, blocks, ra);
        else rows_launch<false>(st, blocks, ra);
        HIP_TRY(hipGetLastError());
        if (pred_out) HIP_TRY(hipMemcpyAsync(pred_out + lo, d_pred, (size_t)rows * 2, hipMemcpyDeviceToHost, st));
        if (rank_out) HIP_TRY(hipMemcpyAsync(rank_out + lo, d_rank, (size_t)rows * 2, hipMemcpyDeviceToHost, st));
    }
    for (int s = 1; s < slots; ++s) HIP_TRY(hipStreamSynchronize(call.st[s]));
    hipStream_t s0 = call.st[0];
    HIP_TRY(hipMemcpyAsync(confusion, d_conf, kk * 8, hipMemcpyDeviceToHost, s0));
    HIP_TRY(hipMemcpyAsync(rank_hist, d_rank_hist, ((size_t)k + 1) * 8, hipMemcpyDeviceToHost, s0));
    HIP_TRY(hipMemcpyAsync(scored_count, d_scored_count, (size_t)k * 8, hipMemcpyDeviceToHost, s0));
    HIP_TRY(hipMemcpyAsync(counts, d_counts, sizeof(*counts), hipMemcpyDeviceToHost, s0));
    HIP_TRY(hipStreamSynchronize(s0));
    if (!auc || counts->n_scored == 0) return TH_OK;

    // ---- step 2: sort the packed own-class scores, keep the key halves, class offsets from scored_count
    for (int64_t c = 0; c < k; ++c) offset[c + 1] = offset[c] + scored_count[c];
    HIP_TRY(hipMemcpyAsync(d_offset, offset.data(), ((size_t)k + 1) * sizeof(long long), hipMemcpyHostToDevice, s0));
    size_t tmp_bytes = 0;
    HIP_TRY(rocprim::radix_sort_keys(nullptr, tmp_bytes, d_packed, d_sorted, (size_t)n, 0u, kSortBits, s0));
    if (int rc = th_alloc_or_fail("th_analyse_classes", &call.mem[1], std::max<size_t>(tmp_bytes, 256))) return rc;
    HIP_TRY(rocprim::radix_sort_keys(call.mem[1], tmp_bytes, d_packed, d_sorted, (size_t)n, 0u, kSortBits, s0));
    const long long n_scored = counts->n_scored;
    hipLaunchKernelGGL(k_positives, dim3((unsigned)((n_scored + kThreads - 1) / kThreads)), dim3(kThreads), 0, s0, d_sorted, d_keys, n_scored);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s0));                  // both streams read the table

    // ---- step 3: the pair sweep over the blocks again (a single block is still resident in slot 0)
    SweepArgs sa{};
    sa.keys = d_keys;
    sa.offset = d_offset;
    sa.u2 = d_u2;
    sa.k = (int)k;
    for (int64_t b = 0; b < n_blocks; ++b) {
        const size_t n_runs = grp.run_lo[b + 1] - grp.run_lo[b], n_order = grp.order_lo[b + 1] - grp.order_lo[b];
        if (!n_runs) continue;
        const int s = (int)(b % slots);
        hipStream_t st = call.st[s];
        unsigned char* slot = slot_of(s);
        const int64_t lo = b * block, rows = std::min(block, n - lo);
        int* d_order = (int*)(slot + o_order);
        Run* d_runs = (Run*)(slot + o_runs);
        if (n_blocks > 1)
            HIP_TRY(hipMemcpyAsync(slot, (const unsigned char*)matrix + lo * row_bytes, rows * row_bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_order, grp.order.data() + grp.order_lo[b], n_order * sizeof(int), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_runs, grp.runs.data() + grp.run_lo[b], n_runs * sizeof(Run), hipMemcpyHostToDevice, st));
        sa.x = slot;
        sa.scored = d_flag + lo;
        sa.order = d_order;
        sa.runs = d_runs;
        if (dtype == TH_F16) hipLaunchKernelGGL((k_pair_sweep<true>), dim3((unsigned)n_runs), dim3(kThreads), 0, st, sa);
        else hipLaunchKernelGGL((k_pair_sweep<false>), dim3((unsigned)n_runs), dim3(kThreads), 0, st, sa);
        HIP_TRY(hipGetLastError());
    }
    for (int s = 1; s < slots; ++s) HIP_TRY(hipStreamSynchronize(call.st[s]));
    HIP_TRY(hipMemcpyAsync(pair_u2, d_u2, kk * 8, hipMemcpyDeviceToHost, s0));
    HIP_TRY(hipStreamSynchronize(s0));
    return TH_OK;
}
