// th_secondary_structure: the secondary structure of a BATCH of protein backbones under the DSSP rule (Kabsch & Sander 1983) — the
// backbone hydrogen bonds of every structure by the electrostatic energy of C=O against N-H, then turns, helices (H, G, I), bridges
// and ladders (B, E) and bends (S) as integer pattern matching on the bond bitmap; per residue a class, its bridge partners, flags
// and bond counts, per structure the totals.  What a design pipeline checks first on a refolded design: did it keep the native's
// helices and strands.
//
//     *** PARITY UNPINNED AGAINST DSSP ***  Neither mkdssp nor PyMOL's dss nor STRIDE is available where this project is built.  The
//     rule — written out in include/timed_hip.h — is this project's reading of the published definition and not their code: every
//     bond counts (no "two best per residue" cap), beta-bulges are not bridged over, the priority is H > E > B > G > I > T > S.
//     Assignments can differ from those programs' at helix ends and sheet edges, and no test can pin them against mkdssp.
//
// k_ss_prepare: one thread per residue decides valid and conn(i) and places the amide hydrogen H(i) (NaN where there is none).
// k_ss_hbonds, the hot path: a work item is (structure, tile of 256 acceptors); a thread owns one acceptor and keeps its C, O and CA
// in registers while the donors of its structure stream through LDS in tiles of 256 (N, H and CA: nine arrays of doubles; every
// lane of a wave reads the same donor: a broadcast, no bank conflict).  A donor without H is staged with a NaN CA and the last tile is
// padded with NaN, so the CA test — squared distance < 81, false for a NaN — is the only guard of the four square roots and four
// divisions.  Per word of 64 donors a thread first runs that test alone on all 64 (broadcast reads, a 64-bit mask of the near ones
// in a register) and then walks down its OWN mask, reading its donors from LDS by index.  With the energy under a branch inside the
// first loop, as k_lddt has its body, a wavefront paid the ~300 instructions of the energy for every donor near ANY of its 64
// acceptors — inside a domain that is every donor — with about an eighth of the lanes active; this way it makes as many rounds as
// its busiest lane has near donors (5.06 -> 3.26 ms for 10 000 structures of 300: profiles/secstruct.txt).  The thread collects the
// bonds of the 64 donors in one 64-bit register and stores it: row = acceptor, bit = donor, both structure-local, so a structure's
// bitmap does not depend on where it sits in the batch.
// k_ss_assign: one thread per residue.  Turns are looked up in the bitmap.  Bridges: every form of a bridge (i, j) needs one of
// hb(i-1, j), hb(i, j), hb(i-1, j+1), hb(i, j+1), so the candidates j are the set bits of rows i-1 and i and of the same rows
// shifted by one — a handful per residue; each is tested in full and, when it is a bridge, its ladder neighbours are.  Bonds
// accepted is the row's popcount.  Bonds donated is a column, and the 64 residues of a wavefront are the 64 bits of the SAME word
// of every row: the wavefront loads that word of 64 rows at once, one row per lane, and counts each bit with a ballot — a 64 x 64
// bit transpose in registers.  There is no second bitmap with the roles exchanged: the build without the column (TH_SS_COLUMN=0)
// bounds what one could save (profiles/secstruct.txt has the measurements, and those of the column read one row at a time).
// k_ss_totals: one wavefront per structure sums the rows into 64-bit integers (integer sums: any order gives the same bytes).
// No atomics; nothing depends on the grid, on arrival order or on a structure's place in the batch: two calls give the same bytes.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <new>
#include <vector>

#include "common.h"
#include "device_math.h"
#include "oneshot.h"

// every float64 product, sum, square root and division below is rounded separately, as the NumPy restatement's are
#pragma clang fp contract(off)

// 1: bonds donated is counted down the column of the bitmap (k_ss_assign).  0: it is left 0 — WRONG output, a timing build only:
// what k_ss_assign costs without the column is the most a second bitmap with the roles exchanged could save (profiles/secstruct.txt).
#ifndef TH_SS_COLUMN
#define TH_SS_COLUMN 1
#endif

namespace {

constexpr int kTile = 256;                     // acceptors per work item = threads per workgroup = donors per LDS tile
constexpr int kWave = 64;
constexpr int kPerBlock = kTile / kWave;       // structures per workgroup of k_ss_totals
constexpr unsigned char kValid = 1, kConn = 2, kHasH = 4;      // the bits of meta[]
constexpr double kCos70 = 0.3420201433256688;

__device__ inline double dist(const double* a, double bx, double by, double bz) {
    const double dx = a[0] - bx, dy = a[1] - by, dz = a[2] - bz;
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

__global__ void __launch_bounds__(kTile) k_ss_prepare(const double* __restrict__ backbone, const int* __restrict__ chain,
                                                      const unsigned char* __restrict__ no_h, const long long* __restrict__ offsets,
                                                      const ThTile* __restrict__ items, double* __restrict__ hxyz, unsigned char* __restrict__ meta) {
    const ThTile it = items[blockIdx.x];
    const long long begin = offsets[it.range], end = offsets[it.range + 1];
    const long long i = begin + (long long)it.tile * kTile + threadIdx.x;
    if (i >= end) return;
    auto valid = [&](long long r) {
        const double* p = backbone + 12 * r;
        return finite3(p) && finite3(p + 3) && finite3(p + 6) && finite3(p + 9);
    };
    auto conn = [&](long long r) {             // the link r -> r + 1; both inside the structure
        if (!valid(r) || !valid(r + 1) || chain[r] != chain[r + 1]) return false;
        const double* c = backbone + 12 * r + 6;
        const double* n = backbone + 12 * (r + 1);
        const double dx = c[0] - n[0], dy = c[1] - n[1], dz = c[2] - n[2];
        return (dx * dx + dy * dy) + dz * dz <= 6.25;
    };
    unsigned char m = valid(i) ? kValid : 0;
    if (i + 1 < end && conn(i)) m |= kConn;
    const double nan = __builtin_nan("");
    double h[3] = {nan, nan, nan};
    if (i > begin && !no_h[i] && conn(i - 1)) {
        const double* c = backbone + 12 * (i - 1) + 6;
        const double* o = c + 3;
        const double* n = backbone + 12 * i;
        const double vx = c[0] - o[0], vy = c[1] - o[1], vz = c[2] - o[2];
        const double norm = sqrt((vx * vx + vy * vy) + vz * vz);
        h[0] = n[0] + vx / norm;
        h[1] = n[1] + vy / norm;
        h[2] = n[2] + vz / norm;
        if (finite3(h)) m |= kHasH;            // a C on its O, or a difference that overflows: no hydrogen
        else h[0] = h[1] = h[2] = nan;
    }
    hxyz[3 * i] = h[0];
    hxyz[3 * i + 1] = h[1];
    hxyz[3 * i + 2] = h[2];
    meta[i] = m;
}

__global__ void __launch_bounds__(kTile) k_ss_hbonds(const double* __restrict__ backbone, const double* __restrict__ hxyz,
                                                     const unsigned char* __restrict__ meta, const long long* __restrict__ offsets,
                                                     const long long* __restrict__ word_start, const ThTile* __restrict__ items,
                                                     unsigned long long* __restrict__ bits) {
    __shared__ __attribute__((aligned(16))) double nx[kTile], ny[kTile], nz[kTile], hx[kTile], hy[kTile], hz[kTile], ax[kTile], ay[kTile], az[kTile];
    const int tid = threadIdx.x;
    const ThTile it = items[blockIdx.x];
    const long long begin = offsets[it.range], end = offsets[it.range + 1];
    const int len = (int)(end - begin), words = (len + kWave - 1) / kWave;
    const int a = it.tile * kTile + tid;       // this thread's acceptor, structure-local
    const bool live = a < len;
    const double nan = __builtin_nan("");
    double ca[3] = {nan, nan, nan}, c[3] = {nan, nan, nan}, o[3] = {nan, nan, nan};
    if (live && (meta[begin + a] & kValid)) {  // an invalid acceptor keeps its NaN CA: near nothing
        const double* p = backbone + 12 * (begin + a);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            ca[k] = p[3 + k];
            c[k] = p[6 + k];
            o[k] = p[9 + k];
        }
    }
    unsigned long long* row = bits + word_start[it.range] + (long long)a * words;       // dereferenced by live threads only
    for (int j0 = 0; j0 < len; j0 += kTile) {
        const int j = j0 + tid;
        const bool donor = j < len && (meta[begin + j] & kHasH);
        const double* p = backbone + 12 * (begin + j);
        const double* h = hxyz + 3 * (begin + j);
        __syncthreads();                       // the previous tile is no longer read
        nx[tid] = donor ? p[0] : nan;
        ny[tid] = donor ? p[1] : nan;
        nz[tid] = donor ? p[2] : nan;
        hx[tid] = donor ? h[0] : nan;
        hy[tid] = donor ? h[1] : nan;
        hz[tid] = donor ? h[2] : nan;
        ax[tid] = donor ? p[3] : nan;
        ay[tid] = donor ? p[4] : nan;
        az[tid] = donor ? p[5] : nan;
        __syncthreads();
        const int groups = ((len - j0 < kTile ? len - j0 : kTile) + kWave - 1) / kWave;     // words of 64 donors in this tile
        for (int g = 0; g < groups; ++g) {
            // first the cheap test on all 64 donors of the word, a broadcast read each: which are near this acceptor
            unsigned long long near = 0;
#pragma unroll 4
            for (int b = 0; b < kWave; b += 2) {
                const int jj = g * kWave + b;
                const double2 x = *(const double2*)&ax[jj], y = *(const double2*)&ay[jj], z = *(const double2*)&az[jj];
                const double dx0 = x.x - ca[0], dy0 = y.x - ca[1], dz0 = z.x - ca[2];
                const double dx1 = x.y - ca[0], dy1 = y.y - ca[1], dz1 = z.y - ca[2];
                near |= (unsigned long long)((dx0 * dx0 + dy0 * dy0) + dz0 * dz0 < 81.0 ? 1 : 0) << b;      // false for a NaN
                near |= (unsigned long long)((dx1 * dx1 + dy1 * dy1) + dz1 * dz1 < 81.0 ? 2 : 0) << b;
            }
            const int first = j0 + g * kWave;  // d != a and d != a + 1
            if (a >= first && a < first + kWave) near &= ~(1ull << (a - first));
            if (a + 1 >= first && a + 1 < first + kWave) near &= ~(1ull << (a + 1 - first));
            // then the energy of the near ones, each lane down its own list: the wavefront makes as many rounds as its busiest lane
            // has near donors, not as many as the donors that are near ANY of its acceptors (measured: profiles/secstruct.txt)
            unsigned long long word = 0;
            while (near) {
                const int b = __builtin_ctzll(near), jj = g * kWave + b;
                near &= near - 1;
                const double r_on = dist(o, nx[jj], ny[jj], nz[jj]), r_ch = dist(c, hx[jj], hy[jj], hz[jj]);
                const double r_oh = dist(o, hx[jj], hy[jj], hz[jj]), r_cn = dist(c, nx[jj], ny[jj], nz[jj]);
                const double q = ((1.0 / r_on + 1.0 / r_ch) - 1.0 / r_oh) - 1.0 / r_cn;
                const double e = floor((27.888 * q) * 1000.0 + 0.5);
                const bool close = r_on < 0.5 || r_ch < 0.5 || r_oh < 0.5 || r_cn < 0.5;
                // a bond: e < -500 milli-kcal/mol, and -9900 when two atoms nearly coincide (e is then not looked at: it may be NaN)
                if (close || e < -500.0) word |= 1ull << b;
            }
            if (live) row[j0 / kWave + g] = word;
        }
    }
}

struct Structure {                             // what k_ss_assign knows of the structure of its residue
    const unsigned long long* bits;
    const unsigned char* meta;                 // of the structure's first residue
    int len, words;
    __device__ bool hb(int acceptor, int donor) const {
        if (acceptor < 0 || donor < 0 || acceptor >= len || donor >= len) return false;
        return (bits[(long long)acceptor * words + (donor >> 6)] >> (donor & 63)) & 1;
    }
    __device__ bool conn(int i) const { return i >= 0 && i < len && (meta[i] & kConn); }
    __device__ bool turn(int i, int n) const {
        if (!hb(i, i + n)) return false;
        for (int k = i; k < i + n; ++k)
            if (!conn(k)) return false;
        return true;
    }
    __device__ bool framed(int i, int j) const {
        const int gap = i < j ? j - i : i - j;
        return gap >= 3 && conn(i - 1) && conn(i) && conn(j - 1) && conn(j);
    }
    __device__ bool parallel(int i, int j) const { return framed(i, j) && ((hb(i - 1, j) && hb(j, i + 1)) || (hb(j - 1, i) && hb(i, j + 1))); }
    __device__ bool antiparallel(int i, int j) const { return framed(i, j) && ((hb(i, j) && hb(j, i)) || (hb(i - 1, j + 1) && hb(j - 1, i + 1))); }
    __device__ unsigned long long word(int row, int w) const { return row < 0 || row >= len || w >= words ? 0ull : bits[(long long)row * words + w]; }
};

__global__ void __launch_bounds__(kTile) k_ss_assign(const double* __restrict__ backbone, const unsigned char* __restrict__ meta,
                                                     const long long* __restrict__ offsets, const long long* __restrict__ word_start,
                                                     const ThTile* __restrict__ items, const unsigned long long* __restrict__ bits,
                                                     unsigned char* __restrict__ class_out, int* __restrict__ residue_out) {
    const ThTile it = items[blockIdx.x];
    const long long begin = offsets[it.range], end = offsets[it.range + 1];
    Structure s;
    s.len = (int)(end - begin);
    s.words = (s.len + kWave - 1) / kWave;
    s.bits = bits + word_start[it.range];
    s.meta = meta + begin;
    const int i = it.tile * kTile + threadIdx.x;
    // Bonds donated, by the whole wavefront before any lane leaves: its 64 residues are the 64 bits of ONE word of every row.  Lane l
    // loads that word of row r0 + l — 64 rows per load instruction — and bit b of the 64 words is counted with one ballot, for lane b.
    int donated = 0;
#if TH_SS_COLUMN
    const int lane = threadIdx.x % kWave, col = (i - lane) >> 6;
    if (col < s.words) {                         // the same for all 64 lanes
        for (int r0 = 0; r0 < s.len; r0 += kWave) {
            const int r = r0 + lane;
            const unsigned long long word = r < s.len ? s.bits[(long long)r * s.words + col] : 0ull;
            if (__ballot(word != 0) == 0) continue;                                         // none of these 64 rows bonds to any of us
#pragma unroll 8
            for (int b = 0; b < kWave; ++b) {
                const int n = __popcll(__ballot((word >> b) & 1));
                donated += lane == b ? n : 0;
            }
        }
    }
#endif
    if (i >= s.len) return;
    const unsigned char m = s.meta[i];
    int flags = (m & kValid ? 128 : 0) | (m & kConn ? 64 : 0);
    bool helix[3], inside = false;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int n = 3 + t;
        if (s.turn(i, n)) flags |= 1 << t;
        helix[t] = false;
        for (int k = i - n + 1; k <= i; ++k) helix[t] = helix[t] || (s.turn(k - 1, n) && s.turn(k, n));
        for (int k = i - n + 1; k < i; ++k) inside = inside || s.turn(k, n);
    }
    // bridges: the candidates are the donors of rows i-1 and i and their left neighbours
    int partner[2] = {-1, -1}, n_partners = 0;
    bool ladder = false;
    if (s.conn(i - 1) && s.conn(i)) {
        unsigned long long here = s.word(i - 1, 0) | s.word(i, 0);
        for (int w = 0; w < s.words; ++w) {
            const unsigned long long next = s.word(i - 1, w + 1) | s.word(i, w + 1);
            unsigned long long cand = here | (here >> 1) | (next << 63);
            here = next;
            while (cand) {
                const int j = w * kWave + __builtin_ctzll(cand);
                cand &= cand - 1;
                const bool p = s.parallel(i, j), a = s.antiparallel(i, j);
                if (!p && !a) continue;
                if (n_partners < 2) partner[n_partners] = j;
                n_partners += 1;
                flags |= (p ? 16 : 0) | (a ? 32 : 0);
                ladder = ladder || (p && (s.parallel(i + 1, j + 1) || s.parallel(i - 1, j - 1))) ||
                         (a && (s.antiparallel(i + 1, j - 1) || s.antiparallel(i - 1, j + 1)));
            }
        }
    }
    if (s.conn(i - 2) && s.conn(i - 1) && s.conn(i) && s.conn(i + 1)) {                     // a bend of more than 70 degrees
        const double* p = backbone + 12 * (begin + i) + 3;
        const double ux = p[0] - p[-24], uy = p[1] - p[-23], uz = p[2] - p[-22];
        const double vx = p[24] - p[0], vy = p[25] - p[1], vz = p[26] - p[2];
        const double dot = (ux * vx + uy * vy) + uz * vz;
        const double nu = sqrt((ux * ux + uy * uy) + uz * uz), nv = sqrt((vx * vx + vy * vy) + vz * vz);
        if (dot / (nu * nv) < kCos70) flags |= 8;                                           // false for a NaN
    }
    int accepted = 0;
    for (int k = 0; k < s.words; ++k) accepted += __builtin_popcountll(s.bits[(long long)i * s.words + k]);
    const int code = helix[1] ? 1 : ladder ? 3 : n_partners ? 2 : helix[0] ? 4 : helix[2] ? 5 : inside ? 6 : (flags & 8) ? 7 : 0;
    class_out[begin + i] = (unsigned char)((m & kValid) ? code : 0);
    int* out = residue_out + 6 * (begin + i);
    out[0] = partner[0];
    out[1] = partner[1];
    out[2] = flags;
    out[3] = accepted;
    out[4] = donated;
    out[5] = n_partners;
}

__global__ void __launch_bounds__(kTile) k_ss_totals(const unsigned char* __restrict__ meta, const long long* __restrict__ offsets,
                                                     long long n_structures, const unsigned char* __restrict__ cls,
                                                     const int* __restrict__ residue, long long* __restrict__ structure_out) {
    const long long s = (long long)blockIdx.x * kPerBlock + threadIdx.x / kWave;
    if (s >= n_structures) return;             // the whole wavefront leaves
    const int lane = threadIdx.x % kWave;
    long long sum[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (long long i = offsets[s] + lane; i < offsets[s + 1]; i += kWave) {
        sum[0] += meta[i] & kValid ? 1 : 0;
        sum[1] += residue[6 * i + 3];
        const int c = cls[i];
#pragma unroll
        for (int k = 0; k < 8; ++k) sum[2 + k] += c == k ? 1 : 0;
    }
#pragma unroll
    for (int k = 0; k < 10; ++k) sum[k] = wave_sum(sum[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 10; ++k) structure_out[10 * s + k] = sum[k];
    }
}

}  // namespace

extern "C" int th_secondary_structure(int device, const double* backbone, const int32_t* chain, const uint8_t* no_h, int64_t total,
                                      const int64_t* offsets, int64_t n_structures, uint8_t* class_out, int32_t* residue_out,
                                      int64_t* structure_out, uint64_t* hbond_bits_out, double* kernel_ms) {
    if (total < 0 || n_structures < 0)
        TH_FAIL(TH_EINVAL, "th_secondary_structure: negative size (total = %lld, n_structures = %lld)", (long long)total, (long long)n_structures);
    if (total > INT_MAX || n_structures > INT_MAX)
        TH_FAIL(TH_EINVAL, "th_secondary_structure: %lld residues / %lld structures in one call (limit 2^31 - 1 each)", (long long)total,
                (long long)n_structures);
    if (n_structures == 0) {
        if (total != 0) TH_FAIL(TH_EINVAL, "th_secondary_structure: n_structures = 0 owns no residue, total = %lld", (long long)total);
        if (kernel_ms) kernel_ms[0] = kernel_ms[1] = kernel_ms[2] = 0.0;
        return TH_OK;
    }
    if (!offsets || !structure_out || (total > 0 && (!backbone || !chain || !no_h || !class_out || !residue_out)))
        TH_FAIL(TH_EINVAL,
                "th_secondary_structure: n_structures = %lld needs offsets and structure_out, total = %lld needs backbone, chain, no_h, "
                "class_out and residue_out", (long long)n_structures, (long long)total);
    if (int rc = th_check_offsets("th_secondary_structure", "offsets", "total", offsets, n_structures, total)) return rc;
    std::vector<ThTile> items;                 // residues offsets[range] + tile * kTile ... of that structure
    if (int rc = th_tile_items("th_secondary_structure", "residues", offsets, n_structures, kTile, items)) return rc;
    std::vector<long long> word_start;
    try {
        word_start.reserve((size_t)n_structures + 1);
        word_start.push_back(0);
        for (int64_t s = 0; s < n_structures; ++s) {
            const int64_t len = offsets[s + 1] - offsets[s];
            word_start.push_back(word_start.back() + len * ((len + kWave - 1) / kWave));   // < 2^31 * 2^25
        }
    } catch (const std::bad_alloc&) {
        TH_FAIL(TH_ENOMEM, "th_secondary_structure: out of host memory for the work items of %lld residues", (long long)total);
    }
    if (word_start.back() > (long long)1 << 50)
        TH_FAIL(TH_ENOMEM, "th_secondary_structure: %lld words of hydrogen-bond bitmap (L * ceil(L / 64) per structure) fit no device", word_start.back());

    const size_t n = (size_t)total, ns = (size_t)n_structures, n_words = (size_t)word_start.back();
    ThLayout lay;
    const size_t o_backbone = lay.take(n * 12 * sizeof(double)), o_chain = lay.take(n * sizeof(int32_t)), o_no_h = lay.take(n);
    const size_t o_offsets = lay.take((ns + 1) * sizeof(int64_t)), o_start = lay.take((ns + 1) * sizeof(long long));
    const size_t o_items = lay.take(items.size() * sizeof(ThTile)), o_h = lay.take(n * 3 * sizeof(double)), o_meta = lay.take(n);
    const size_t o_bits = lay.take(n_words * sizeof(uint64_t)), o_class = lay.take(n), o_res = lay.take(n * 6 * sizeof(int32_t));
    const size_t o_struct = lay.take(ns * 10 * sizeof(int64_t));
    ThCall call;
    if (int rc = call.open("th_secondary_structure", device, lay.bytes, kernel_ms ? 4 : 0)) return rc;
    double *d_backbone = call.at<double>(o_backbone), *d_h = call.at<double>(o_h);
    int *d_chain = call.at<int>(o_chain), *d_res = call.at<int>(o_res);
    unsigned char *d_no_h = call.at<unsigned char>(o_no_h), *d_meta = call.at<unsigned char>(o_meta), *d_class = call.at<unsigned char>(o_class);
    long long *d_offsets = call.at<long long>(o_offsets), *d_start = call.at<long long>(o_start), *d_struct = call.at<long long>(o_struct);
    unsigned long long* d_bits = call.at<unsigned long long>(o_bits);
    ThTile* d_items = call.at<ThTile>(o_items);
    hipStream_t st = call.st[0];
    if (n) {
        HIP_TRY(hipMemcpyAsync(d_backbone, backbone, n * 12 * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_chain, chain, n * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_no_h, no_h, n, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(ThTile), hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipMemcpyAsync(d_offsets, offsets, (ns + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_start, word_start.data(), (ns + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
    const dim3 grid((unsigned)items.size()), block(kTile);
    HIP_TRY(call.mark(0));
    if (!items.empty()) {
        hipLaunchKernelGGL(k_ss_prepare, grid, block, 0, st, d_backbone, d_chain, d_no_h, d_offsets, d_items, d_h, d_meta);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_ss_hbonds, grid, block, 0, st, d_backbone, d_h, d_meta, d_offsets, d_start, d_items, d_bits);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(call.mark(1));
    if (!items.empty()) {
        hipLaunchKernelGGL(k_ss_assign, grid, block, 0, st, d_backbone, d_meta, d_offsets, d_start, d_items, d_bits, d_class, d_res);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(call.mark(2));
    hipLaunchKernelGGL(k_ss_totals, dim3((unsigned)((ns + kPerBlock - 1) / kPerBlock)), block, 0, st, d_meta, d_offsets, (long long)n_structures,
                       d_class, d_res, d_struct);
    HIP_TRY(hipGetLastError());
    HIP_TRY(call.mark(3));
    if (n) {
        HIP_TRY(hipMemcpyAsync(class_out, d_class, n, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(residue_out, d_res, n * 6 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    if (hbond_bits_out && n_words) HIP_TRY(hipMemcpyAsync(hbond_bits_out, d_bits, n_words * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(structure_out, d_struct, ns * 10 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    return call.finish(kernel_ms, 3);
}
