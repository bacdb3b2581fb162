// th_packing_density: atomic contact number ("packing density", Weiss 2007) of every atom of a BATCH of structures, and its
// per-residue summary — what the reference computes per structure with a NumPy loop over atoms (design_utils/analyse_utils.py
// tag_packing_density :78-86, _extract_packdensity_from_polypeptide :176-201):
//     density[i] = #{ j in the structure of i, j == i included : sqrt((dx*dx + dy*dy) + dz*dz) < radius } - 1
// in float64, in that summation order, every product and sum rounded on its own (no fused multiply-add): the answer is an integer
// and has to land on the reference's side of every tie, so the arithmetic is the reference's term for term.
//
// The square root is not taken.  sqrt is monotone, so there is one threshold T(radius) with  sqrt_rn(s) < radius  <=>  s < T  for
// EVERY double s: the smallest s whose correctly rounded root reaches the radius.  T is not radius * radius in general (the root
// of the predecessor of fl(r^2) can round back up to r); th_packing_threshold finds it on the host by walking the neighbours of
// r^2 with the host's IEEE square root, and the kernel compares the squared distance with it.
//
// k_contacts, the hot path: a work item is (structure, tile of 256 atoms i); a thread owns one atom i and keeps its count in a
// register while the atoms j of its structure stream through LDS in tiles of 256 (three arrays of doubles; every lane of a wave
// reads the same j: a broadcast, no bank conflict).  The last tile is padded with NaN coordinates, which never count, so the
// inner loop has no bounds test.  No atomics, no dependence on the grid or on arrival order: two calls give the same bytes.  Two
// thousand 2 500-atom structures (20 000 work items) and one 100 000-atom assembly (391) both come from one launch.
// k_residues: a thread per residue folds the counts of its selected atoms in file order with the reference's running half-average.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>
#include <limits>
#include <new>
#include <vector>

#include "common.h"
#include "oneshot.h"

// every float64 product and sum below is rounded separately, as NumPy's are
#pragma clang fp contract(off)

namespace {

constexpr int kTile = 256;                     // atoms i per work item = threads per workgroup = atoms j per LDS tile

struct Item { int begin, end, i0; };           // the structure's atoms [begin, end), this item's atoms [i0, min(i0 + kTile, end))
struct Span { int start, count; };             // a residue's atoms (contiguous in the batch)

__global__ void __launch_bounds__(kTile) k_contacts(const double* __restrict__ xyz, const Item* __restrict__ items, double threshold,
                                                    int* __restrict__ density) {
    __shared__ __attribute__((aligned(16))) double sx[kTile], sy[kTile], sz[kTile];
    const int tid = threadIdx.x;
    const Item it = items[blockIdx.x];
    const int i = it.i0 + tid;
    const bool live = i < it.end;
    const double nan = __builtin_nan("");
    const double xi = live ? xyz[3 * (size_t)i] : nan, yi = live ? xyz[3 * (size_t)i + 1] : nan, zi = live ? xyz[3 * (size_t)i + 2] : nan;
    int count = 0;
    for (int j0 = it.begin; j0 < it.end; j0 += kTile) {
        const int j = j0 + tid;
        const bool have = j < it.end;
        const double a = have ? xyz[3 * (size_t)j] : nan, b = have ? xyz[3 * (size_t)j + 1] : nan, c = have ? xyz[3 * (size_t)j + 2] : nan;
        __syncthreads();                       // the previous tile is no longer read
        sx[tid] = a;
        sy[tid] = b;
        sz[tid] = c;
        __syncthreads();
        const int m = min(kTile, it.end - j0), m4 = (m + 3) & ~3;      // slots m .. m4 hold NaN
#pragma unroll 2
        for (int jj = 0; jj < m4; jj += 4) {
            const double2 x0 = *(const double2*)&sx[jj], x1 = *(const double2*)&sx[jj + 2];
            const double2 y0 = *(const double2*)&sy[jj], y1 = *(const double2*)&sy[jj + 2];
            const double2 z0 = *(const double2*)&sz[jj], z1 = *(const double2*)&sz[jj + 2];
            const double xs[4] = {x0.x, x0.y, x1.x, x1.y}, ys[4] = {y0.x, y0.y, y1.x, y1.y}, zs[4] = {z0.x, z0.y, z1.x, z1.y};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const double dx = xs[u] - xi, dy = ys[u] - yi, dz = zs[u] - zi;
                const double s = (dx * dx + dy * dy) + dz * dz;
                count += s < threshold ? 1 : 0;                        // false for a NaN
            }
        }
    }
    if (live) density[i] = count - 1;          // the atom counted itself (unless a coordinate is not finite or radius <= 0: -1)
}

// the reference's per-residue value: -1 until the first selected atom, then cur = (cur + next) / 2 in file order — with its own
// test `cur == -1` for "nothing yet", so selected atoms whose count is -1 (a non-finite coordinate) are skipped while they lead
__global__ void __launch_bounds__(kTile) k_residues(const int* __restrict__ density, const unsigned char* __restrict__ selected,
                                                    const Span* __restrict__ spans, long long n_groups, double* __restrict__ out) {
    const long long g = (long long)blockIdx.x * kTile + threadIdx.x;
    if (g >= n_groups) return;
    const Span sp = spans[g];
    double cur = -1.0;
    for (int a = sp.start; a < sp.start + sp.count; ++a) {
        if (!selected[a]) continue;
        const double d = (double)density[a];
        cur = cur == -1.0 ? d : (cur + d) / 2;
    }
    out[g] = cur;
}

}  // namespace

extern "C" double th_packing_threshold(double radius) {
    if (radius != radius) return radius;                   // s < NaN is never true, as sqrt(s) < NaN
    if (!(radius > 0)) return 0.0;                          // sqrt(s) >= 0 >= radius; s is a sum of squares, never below +0
    if (std::isinf(radius)) return radius;                  // every finite s
    double t = radius * radius;                             // may round to +inf or to 0
    while (t > 0) {                                         // down while the predecessor's root still reaches the radius
        const double p = std::nextafter(t, 0.0);
        if (!(std::sqrt(p) >= radius)) break;
        t = p;
    }
    while (std::sqrt(t) < radius) t = std::nextafter(t, std::numeric_limits<double>::infinity());
    return t;                                               // the smallest double whose root is >= radius
}

extern "C" int th_packing_density(int device, const double* xyz, int64_t total, const int64_t* offsets, int64_t n_structures,
                                  double radius, const int32_t* group, const uint8_t* selected, int64_t n_groups,
                                  int32_t* density_out, double* residue_out, double* kernel_ms_out) {
    if (total < 0 || n_structures < 0 || n_groups < 0 || !offsets || (total > 0 && !xyz))
        TH_FAIL(TH_EINVAL, "th_packing_density: bad argument");
    if (n_groups > 0 && (!residue_out || (total > 0 && (!group || !selected))))
        TH_FAIL(TH_EINVAL, "th_packing_density: n_groups = %lld needs group, selected and residue_out", (long long)n_groups);
    if (total > INT_MAX - kTile || n_groups > INT_MAX)
        TH_FAIL(TH_EINVAL, "th_packing_density: %lld atoms / %lld residues in one call (limit 2^31 - 257)", (long long)total, (long long)n_groups);
    if (int rc = th_check_offsets("th_packing_density", "offsets", "total", offsets, n_structures, total)) return rc;
    std::vector<Span> spans;
    std::vector<Item> items;
    try {
        spans.assign((size_t)n_groups, Span{0, 0});
        for (int64_t i = 0; n_groups > 0 && i < total; ++i) {
            const int32_t g = group[i];
            if (g < -1 || g >= n_groups) TH_FAIL(TH_EINVAL, "th_packing_density: group[%lld] = %d outside -1..%lld", (long long)i, (int)g, (long long)n_groups - 1);
            if (g < 0) continue;
            Span& sp = spans[(size_t)g];
            if (sp.count == 0) sp.start = (int)i;
            else if (sp.start + sp.count != i)
                TH_FAIL(TH_EINVAL, "th_packing_density: the atoms of residue %d are not contiguous (atom %lld)", (int)g, (long long)i);
            ++sp.count;
        }
        for (int64_t s = 0; s < n_structures; ++s)
            for (int64_t i0 = offsets[s]; i0 < offsets[s + 1]; i0 += kTile) items.push_back(Item{(int)offsets[s], (int)offsets[s + 1], (int)i0});
    } catch (const std::bad_alloc&) {
        TH_FAIL(TH_ENOMEM, "th_packing_density: out of host memory for %lld atoms", (long long)total);
    }
    if (kernel_ms_out) *kernel_ms_out = 0.0;
    if (total == 0) {                                       // nothing to launch: every residue is empty
        for (int64_t g = 0; g < n_groups; ++g) residue_out[g] = -1.0;
        return TH_OK;
    }

    const size_t n = (size_t)total, ng = (size_t)n_groups;
    ThLayout lay;
    const size_t o_xyz = lay.take(n * 3 * sizeof(double)), o_density = lay.take(n * sizeof(int)), o_items = lay.take(items.size() * sizeof(Item));
    const size_t o_sel = lay.take(ng ? n : 0), o_spans = lay.take(ng * sizeof(Span)), o_res = lay.take(ng * sizeof(double));
    ThCall call;
    if (int rc = call.open("th_packing_density", device, lay.bytes, kernel_ms_out ? 2 : 0)) return rc;
    double *d_xyz = call.at<double>(o_xyz), *d_res = call.at<double>(o_res);
    int* d_density = call.at<int>(o_density);
    Item* d_items = call.at<Item>(o_items);
    unsigned char* d_sel = call.at<unsigned char>(o_sel);
    Span* d_spans = call.at<Span>(o_spans);
    hipStream_t st = call.st[0];
    HIP_TRY(hipMemcpyAsync(d_xyz, xyz, n * 3 * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(Item), hipMemcpyHostToDevice, st));
    if (ng) {
        HIP_TRY(hipMemcpyAsync(d_sel, selected, n, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_spans, spans.data(), ng * sizeof(Span), hipMemcpyHostToDevice, st));
    }
    HIP_TRY(call.mark(0));
    hipLaunchKernelGGL(k_contacts, dim3((unsigned)items.size()), dim3(kTile), 0, st, d_xyz, d_items, th_packing_threshold(radius), d_density);
    HIP_TRY(hipGetLastError());
    if (ng) {
        hipLaunchKernelGGL(k_residues, dim3((unsigned)((ng + kTile - 1) / kTile)), dim3(kTile), 0, st, d_density, d_sel, d_spans, (long long)ng, d_res);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(call.mark(1));
    if (density_out) HIP_TRY(hipMemcpyAsync(density_out, d_density, n * sizeof(int), hipMemcpyDeviceToHost, st));
    if (ng) HIP_TRY(hipMemcpyAsync(residue_out, d_res, ng * sizeof(double), hipMemcpyDeviceToHost, st));
    return call.finish(kernel_ms_out);
}
