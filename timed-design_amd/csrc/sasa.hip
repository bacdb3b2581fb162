// th_sasa: the solvent-accessible surface of a BATCH of structures by Shrake & Rupley (1973) — every atom carries a sphere of radius
// R = van der Waals radius + probe with n_points test points on it, and a point is exposed unless it lies strictly inside the sphere
// of another atom of the same structure.  Per atom the number of exposed points and (on request) which ones, per structure the totals;
// areas are the caller's float64 arithmetic on these integers.  Which residues of a design are buried and which face the solvent.
//
//     *** PARITY UNPINNED AGAINST FREESASA / NACCESS / DSSP / BIOPYTHON ***  None of them is available where this project is built.
//     The rule — written out in include/timed_hip.h — is this project's own: the caller's points, strict inequalities, a point exactly
//     on a neighbour's sphere exposed, element radii (the caller's).  Areas differ from those programs' with their radii and points.
//
// k_sasa_points, the hot path: a work item is (structure, four consecutive atoms); a wavefront owns one atom, a lane the points
// lane, lane + 64, ... of it, SLOTS of them at a time in registers (1 up to 64 points, 2 up to 128, else 4: rounds of 64 * SLOTS
// points).  The atoms of the structure stream through LDS in tiles of 256 (x, y, z, R and R * R; an invalid atom is staged with a NaN
// R and is near nothing); the four wavefronts share a tile.  Per 64 candidates each lane tests near(i, j) for one of them, one ballot
// makes that a wave-uniform mask, and the set bits are walked: the candidate is read from LDS by all lanes at once (a broadcast) and
// every lane tests its own points against it.  There is no neighbour list and so no capacity: 300 atoms on one spot are 300 set bits.
// The result is an AND over neighbours, so a wavefront whose points are all buried stops testing (TH_SASA_EARLY_EXIT; it still
// stages and waits with its workgroup), and a workgroup all of whose wavefronts have stopped leaves the tile loop.  The mask word of
// 64 points is the ballot of their flags, the count the popcount of those ballots: integers, no float is reduced.
// k_sasa_totals: one wavefront per structure sums the counts into 64-bit integers (any order gives the same bytes).
// No atomics; nothing depends on the grid, on arrival order or on a structure's place in the batch: two calls give the same bytes.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <new>
#include <vector>

#include "common.h"
#include "device_math.h"
#include "oneshot.h"

// every float64 product, sum and difference below is rounded separately, as the NumPy restatement's are
#pragma clang fp contract(off)

// 1: a wavefront whose points are all buried tests no further candidate.  0: it goes on to the end of its structure — the same
// bytes, a timing build only (profiles/sasa.txt).
#ifndef TH_SASA_EARLY_EXIT
#define TH_SASA_EARLY_EXIT 1
#endif

// atoms per work item, one per wavefront: the wavefronts that share an LDS tile.  4 is the product; 8 and 16 were measured against it
// (profiles/sasa.txt).
#ifndef TH_SASA_ATOMS
#define TH_SASA_ATOMS 4
#endif

namespace {

constexpr int kWave = 64;
constexpr int kAtoms = TH_SASA_ATOMS;          // also the structures per workgroup of k_sasa_totals
constexpr int kTile = kAtoms * kWave;          // candidates per LDS tile = threads per workgroup
constexpr int kMaxPoints = 1024;
constexpr long long kMaxTotal = 2147483647LL - 256;

template <int SLOTS>
__global__ void __launch_bounds__(kTile) k_sasa_points(const double* __restrict__ xyz, const double* __restrict__ radius, double probe,
                                                       const long long* __restrict__ offsets, const ThTile* __restrict__ items,
                                                       const double* __restrict__ points, int n_points, int words,
                                                       int* __restrict__ exposed_out, unsigned long long* __restrict__ mask_out) {
    __shared__ __attribute__((aligned(16))) double cx[kTile], cy[kTile], cz[kTile], cr[kTile], crr[kTile];
    const int tid = threadIdx.x, lane = tid % kWave;
    const ThTile it = items[blockIdx.x];                          // atoms offsets[range] + tile * kAtoms ... of that structure
    const long long begin = offsets[it.range], end = offsets[it.range + 1];
    const int len = (int)(end - begin);
    const int a = it.tile * kAtoms + tid / kWave;                 // this wavefront's atom, structure-local
    const bool live = a < len;                                    // the same for all 64 lanes
    const double nan = __builtin_nan("");
    double x = nan, y = nan, z = nan, R = nan;
    if (live) {
        const double* p = xyz + 3 * (begin + a);
        x = p[0];
        y = p[1];
        z = p[2];
        R = radius[begin + a] + probe;
    }
    const bool valid = finite3(x, y, z) && __builtin_isfinite(R) && R > 0.0;
    int count = 0;
    for (int k0 = 0; k0 < n_points; k0 += kWave * SLOTS) {        // a round: points k0 + lane + 64 * s
        double px[SLOTS], py[SLOTS], pz[SLOTS];
        bool open[SLOTS];                                         // not buried so far
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            const int k = k0 + s * kWave + lane;
            open[s] = valid && k < n_points;
            const double* u = points + 3 * (k < n_points ? k : 0);
            px[s] = x + R * u[0];
            py[s] = y + R * u[1];
            pz[s] = z + R * u[2];
        }
        bool testing = valid;                                     // wave-uniform: some point of this round is still open
        for (int j0 = 0; j0 < len; j0 += kTile) {
            const int j = j0 + tid;
            double qx = nan, qy = nan, qz = nan, qr = nan;
            if (j < len) {
                const double* p = xyz + 3 * (begin + j);
                qx = p[0];
                qy = p[1];
                qz = p[2];
                qr = radius[begin + j] + probe;
                // finite3(qx, qy, qz) spelled out: through the function hipcc folds the chain into selects before it inlines, and
                // this loop's code and registers change (2 SGPRs at SLOTS 2 and 4) — not in a change that promises the same kernel
                if (!(__builtin_isfinite(qx) && __builtin_isfinite(qy) && __builtin_isfinite(qz) && __builtin_isfinite(qr) && qr > 0.0)) qr = nan;
            }
            if (!__syncthreads_or(testing)) break;                // the previous tile is no longer read; nobody has anything left to test
            cx[tid] = qx;
            cy[tid] = qy;
            cz[tid] = qz;
            cr[tid] = qr;
            crr[tid] = qr * qr;
            __syncthreads();
            if (!testing) continue;
            const int groups = ((len - j0 < kTile ? len - j0 : kTile) + kWave - 1) / kWave;
            for (int g = 0; g < groups; ++g) {
                const int jj = g * kWave + lane;                  // each lane tests near(a, j) for one candidate; a NaN R is near nothing
                const double dx = cx[jj] - x, dy = cy[jj] - y, dz = cz[jj] - z;
                const double s2 = (dx * dx + dy * dy) + dz * dz, t = R + cr[jj];
                unsigned long long near = __ballot(s2 < t * t && j0 + jj != a);
                while (near) {                                    // uniform: every lane reads the same candidate, a broadcast
                    const int b = g * kWave + __builtin_ctzll(near);
                    near &= near - 1;
                    const double ox = cx[b], oy = cy[b], oz = cz[b], orr = crr[b];
#pragma unroll
                    for (int s = 0; s < SLOTS; ++s) {
                        const double ex = px[s] - ox, ey = py[s] - oy, ez = pz[s] - oz;
                        if ((ex * ex + ey * ey) + ez * ez < orr) open[s] = false;
                    }
                }
#if TH_SASA_EARLY_EXIT
                bool any = false;
#pragma unroll
                for (int s = 0; s < SLOTS; ++s) any = any || open[s];
                if (__ballot(any) == 0) {
                    testing = false;
                    break;
                }
#endif
            }
        }
        __syncthreads();                                          // the next round stages again
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            const unsigned long long word = __ballot(open[s]);
            count += __popcll(word);
            const int w = k0 / kWave + s;
            if (mask_out && live && lane == 0 && w < words) mask_out[(begin + a) * words + w] = word;
        }
    }
    if (live && lane == 0) exposed_out[begin + a] = valid ? count : -1;
}

__global__ void __launch_bounds__(kTile) k_sasa_totals(const long long* __restrict__ offsets, long long n_structures,
                                                       const int* __restrict__ exposed, long long* __restrict__ structure_out) {
    const long long s = (long long)blockIdx.x * kAtoms + threadIdx.x / kWave;
    if (s >= n_structures) return;             // the whole wavefront leaves
    const int lane = threadIdx.x % kWave;
    long long n_valid = 0, n_buried = 0, sum = 0;
    for (long long i = offsets[s] + lane; i < offsets[s + 1]; i += kWave) {
        const int e = exposed[i];
        n_valid += e >= 0 ? 1 : 0;
        n_buried += e == 0 ? 1 : 0;
        sum += e > 0 ? e : 0;
    }
    n_valid = wave_sum(n_valid);
    n_buried = wave_sum(n_buried);
    sum = wave_sum(sum);
    if (lane == 0) {
        structure_out[3 * s] = n_valid;
        structure_out[3 * s + 1] = n_buried;
        structure_out[3 * s + 2] = sum;
    }
}

}  // namespace

extern "C" int th_sasa_sphere(int32_t n_points, double* points_out) {
    if (n_points < 1 || n_points > kMaxPoints) TH_FAIL(TH_EINVAL, "th_sasa_sphere: n_points = %d is outside 1 .. %d", (int)n_points, kMaxPoints);
    if (!points_out) TH_FAIL(TH_EINVAL, "th_sasa_sphere: points_out is NULL");
    const double pi = 3.141592653589793, step = pi * (3.0 - sqrt(5.0)), n = (double)n_points;
    for (int k = 0; k < n_points; ++k) {
        const double z = 1.0 - (double)(2 * k + 1) / n, rho = sqrt(1.0 - z * z), phi = (double)k * step;
        points_out[3 * k] = rho * cos(phi);
        points_out[3 * k + 1] = rho * sin(phi);
        points_out[3 * k + 2] = z;
    }
    return TH_OK;
}

extern "C" int th_sasa(int device, const double* xyz, const double* radius, int64_t total, const int64_t* offsets, int64_t n_structures,
                       double probe, const double* points, int32_t n_points, int32_t* exposed_out, uint64_t* mask_out, int64_t* structure_out,
                       double* kernel_ms_out) {
    if (total < 0 || n_structures < 0)
        TH_FAIL(TH_EINVAL, "th_sasa: negative size (total = %lld, n_structures = %lld)", (long long)total, (long long)n_structures);
    if (total > kMaxTotal || n_structures > INT_MAX)
        TH_FAIL(TH_EINVAL, "th_sasa: %lld atoms / %lld structures in one call (limits 2^31 - 257 and 2^31 - 1)", (long long)total, (long long)n_structures);
    if (n_points < 1 || n_points > kMaxPoints) TH_FAIL(TH_EINVAL, "th_sasa: n_points = %d is outside 1 .. %d", (int)n_points, kMaxPoints);
    if (!points) TH_FAIL(TH_EINVAL, "th_sasa: points is NULL");
    for (int k = 0; k < 3 * n_points; ++k)
        if (!std::isfinite(points[k])) TH_FAIL(TH_EINVAL, "th_sasa: coordinate %d of point %d is not finite", k % 3, k / 3);
    if (n_structures == 0) {
        if (total != 0) TH_FAIL(TH_EINVAL, "th_sasa: n_structures = 0 owns no atom, total = %lld", (long long)total);
        if (kernel_ms_out) kernel_ms_out[0] = kernel_ms_out[1] = 0.0;
        return TH_OK;
    }
    if (!offsets || !structure_out || (total > 0 && (!xyz || !radius || !exposed_out)))
        TH_FAIL(TH_EINVAL, "th_sasa: n_structures = %lld needs offsets and structure_out, total = %lld needs xyz, radius and exposed_out",
                (long long)n_structures, (long long)total);
    if (int rc = th_check_offsets("th_sasa", "offsets", "total", offsets, n_structures, total)) return rc;
    if (total == 0) {                          // structures without atoms: nothing to launch
        for (int64_t k = 0; k < 3 * n_structures; ++k) structure_out[k] = 0;
        if (kernel_ms_out) kernel_ms_out[0] = kernel_ms_out[1] = 0.0;
        return TH_OK;
    }
    std::vector<ThTile> items;
    if (int rc = th_tile_items("th_sasa", "atoms", offsets, n_structures, kAtoms, items)) return rc;

    const size_t n = (size_t)total, ns = (size_t)n_structures, words = ((size_t)n_points + 63) / 64;
    ThLayout lay;
    const size_t o_xyz = lay.take(n * 3 * sizeof(double)), o_radius = lay.take(n * sizeof(double));
    const size_t o_offsets = lay.take((ns + 1) * sizeof(int64_t)), o_items = lay.take(items.size() * sizeof(ThTile));
    const size_t o_points = lay.take((size_t)n_points * 3 * sizeof(double)), o_exposed = lay.take(n * sizeof(int32_t));
    const size_t o_mask = lay.take(mask_out ? n * words * sizeof(uint64_t) : 0), o_struct = lay.take(ns * 3 * sizeof(int64_t));
    ThCall call;
    if (int rc = call.open("th_sasa", device, lay.bytes, kernel_ms_out ? 3 : 0)) return rc;
    double *d_xyz = call.at<double>(o_xyz), *d_radius = call.at<double>(o_radius), *d_points = call.at<double>(o_points);
    long long *d_offsets = call.at<long long>(o_offsets), *d_struct = call.at<long long>(o_struct);
    int* d_exposed = call.at<int>(o_exposed);
    unsigned long long* d_mask = mask_out ? call.at<unsigned long long>(o_mask) : nullptr;
    ThTile* d_items = call.at<ThTile>(o_items);
    hipStream_t st = call.st[0];
    HIP_TRY(hipMemcpyAsync(d_xyz, xyz, n * 3 * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_radius, radius, n * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_offsets, offsets, (ns + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(ThTile), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_points, points, (size_t)n_points * 3 * sizeof(double), hipMemcpyHostToDevice, st));
    const dim3 grid((unsigned)items.size()), block(kTile);
    HIP_TRY(call.mark(0));
    if (n_points <= kWave)
        hipLaunchKernelGGL(k_sasa_points<1>, grid, block, 0, st, d_xyz, d_radius, probe, d_offsets, d_items, d_points, (int)n_points, (int)words,
                           d_exposed, d_mask);
    else if (n_points <= 2 * kWave)
        hipLaunchKernelGGL(k_sasa_points<2>, grid, block, 0, st, d_xyz, d_radius, probe, d_offsets, d_items, d_points, (int)n_points, (int)words,
                           d_exposed, d_mask);
    else
        hipLaunchKernelGGL(k_sasa_points<4>, grid, block, 0, st, d_xyz, d_radius, probe, d_offsets, d_items, d_points, (int)n_points, (int)words,
                           d_exposed, d_mask);
    HIP_TRY(hipGetLastError());
    HIP_TRY(call.mark(1));
    hipLaunchKernelGGL(k_sasa_totals, dim3((unsigned)((ns + kAtoms - 1) / kAtoms)), block, 0, st, d_offsets, (long long)n_structures, d_exposed,
                       d_struct);
    HIP_TRY(hipGetLastError());
    HIP_TRY(call.mark(2));
    HIP_TRY(hipMemcpyAsync(exposed_out, d_exposed, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (mask_out) HIP_TRY(hipMemcpyAsync(mask_out, d_mask, n * words * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(structure_out, d_struct, ns * 3 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    return call.finish(kernel_ms_out, 2);
}
