// GPU voxeliser: atoms + one local frame per residue -> voxel frames [n_frames, V, V, V, C], the input of the
// CNN (what aposteriori.make_frame_dataset produces for the reference: ui.py:73-86, README.md:83-97; dataset layout
// design_utils/utils.py:238-251).  ONE kernel and one host path behind both entry points: th_voxelise_batch takes the frames of MANY
// structures in one launch, optionally with a weight per atom (the property channel of timed_hip/voxeliser.py spec item 8: a charge
// or polarity value at a residue's CA); th_voxelise is its one-structure case without weights.
//
// PARITY UNPINNED AGAINST AMPAL AND APOSTERIORI (aposteriori==2.4.0's source is not in the reference tree): the frames follow the
// specification written out in timed_hip/voxeliser.py (items 3-6 and 8) and are tested against its NumPy restatement
// (oracle/voxel_oracle.py) — bit-exact for boolean frames, to exp() rounding for Gaussian ones.
//
// Rule.  Frame r sees the atoms [atom_offsets[s], atom_offsets[s + 1]) of structure s = frame_structure[r] and no others.  One
// workgroup per frame.  Phase 1 walks that atom range in order, 256 atoms per pass starting AT the range's first atom (which is
// no multiple of 256 in the flat arrays), transforms each atom into the frame (float32, separate multiplies and adds: no FMA
// contraction, so the host restatement reproduces the indices bit for bit) and keeps those whose voxel lies inside the cube in an
// LDS list by an ordered compaction (wave ballots + a per-chunk wave prefix): the list is in atom order.  Phase 2 is a GATHER: a
// thread owns voxels and sums the listed atoms' contributions in list order, acc = acc + weight * (w / total) with the quotient, the
// product and the sum each rounded to float32 (no contraction) — deterministic, where a scatter with float atomics would make
// overlapping Gaussians of neighbouring backbone atoms order-dependent.  The list is binned by x-plane first and a voxel walks only
// the atoms within one plane of it, still in list order (a walk of the whole list would skip all the others: the sums see the same
// terms in the same order).  weight is 1.0f when no weights are given, and 1.0f * x is x.  No atomics on frame data: a frame's
// bytes depend on its own atom range and its own frames_rt row only, not on its place in the batch.  A 21 A cube holds 150-250
// encodable atoms; the list holds 2048.
#include "common.h"
#include "oneshot.h"

#include <cmath>
#include <limits.h>
#include <mutex>
#include <utility>
#include <vector>

namespace {

constexpr int kMaxList = 2048;

struct VoxBatchArgs {
    const float* xyz; const int* chn; const float* sig; const float* wgt;       // wgt may be null: every atom counts 1
    const long long* offsets; const int* frame_structure;
    const float* frt; int V; float a; int C; int gaussian;
    void* out; int* overflow;
};

__global__ void __launch_bounds__(256) k_voxelise_batch(const VoxBatchArgs p) {
#pragma clang fp contract(off)
    __shared__ float Lx[kMaxList], Ly[kMaxList], Lz[kMaxList], Lk[kMaxList], Lt[kMaxList], Lw[kMaxList];   // local xyz, 1/(2 sigma^2), sum of the 27 weights, atom weight
    __shared__ int Li[kMaxList];          // (ch << 27) | (i0 << 18) | (i1 << 9) | i2: 3 bits of channel, 9 bits per index
    __shared__ int wave_cnt[4];
    __shared__ int Ps[512];               // V + 1 plane starts into Lp
    __shared__ unsigned short Lp[kMaxList];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = blockIdx.x, V = p.V, centre = V / 2;
    const int s = p.frame_structure[r];
    const long long first = p.offsets[s], last = p.offsets[s + 1];
    const float* F = p.frt + (size_t)r * 12;
    const float R00 = F[0], R01 = F[1], R02 = F[2], R10 = F[3], R11 = F[4], R12 = F[5], R20 = F[6], R21 = F[7], R22 = F[8];
    const float c0 = F[9], c1 = F[10], c2 = F[11];
    int count = 0;
    for (long long base = first; base < last; base += 256) {
        const long long ai = base + tid;
        bool ok = false;
        float l0 = 0.f, l1 = 0.f, l2 = 0.f;
        int i0 = 0, i1 = 0, i2 = 0, ch = 0;
        if (ai < last) {
            const float d0 = p.xyz[3 * ai] - c0, d1 = p.xyz[3 * ai + 1] - c1, d2 = p.xyz[3 * ai + 2] - c2;
            l0 = (R00 * d0 + R01 * d1) + R02 * d2;
            l1 = (R10 * d0 + R11 * d1) + R12 * d2;
            l2 = (R20 * d0 + R21 * d1) + R22 * d2;
            // inside or not is decided on the floored float, with ordered comparisons: NaN and infinity are outside, and only a
            // small integer is ever converted (the conversion turns NaN into 0, the centre voxel, and saturates beyond 2^31)
            const float q0 = floorf(l0 / p.a + 0.5f), q1 = floorf(l1 / p.a + 0.5f), q2 = floorf(l2 / p.a + 0.5f);
            const float lo = (float)(-centre), hi = (float)(V - 1 - centre);
            ch = p.chn[ai];
            ok = q0 >= lo && q0 <= hi && q1 >= lo && q1 <= hi && q2 >= lo && q2 <= hi && ch >= 0 && ch < p.C;
            if (ok) { i0 = (int)q0 + centre; i1 = (int)q1 + centre; i2 = (int)q2 + centre; }
        }
        const unsigned long long mask = __ballot(ok);
        const int before = __popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) wave_cnt[wave] = __popcll(mask);
        __syncthreads();
        int off = count + before;
        for (int w = 0; w < wave; ++w) off += wave_cnt[w];
        const int chunk_total = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        if (ok && off < kMaxList) {
            Lx[off] = l0; Ly[off] = l1; Lz[off] = l2;
            Li[off] = (ch << 27) | (i0 << 18) | (i1 << 9) | i2;
            const float sg = p.gaussian ? p.sig[ai] : 1.f;
            Lk[off] = 1.0f / (2.0f * sg * sg);
            Lw[off] = p.wgt ? p.wgt[ai] : 1.0f;
        }
        count += chunk_total;
        __syncthreads();
    }
    if (count > kMaxList) { if (tid == 0) atomicMax(p.overflow, count); count = kMaxList; }      // an int flag, not frame data
    // the 27 weights of an atom sum to Lt (added in the fixed order axis0, axis1, axis2 outer to inner)
    if (p.gaussian) {
        for (int e = tid; e < count; e += 256) {
            const int pk = Li[e];
            const int i0 = (pk >> 18) & 511, i1 = (pk >> 9) & 511, i2 = pk & 511;
            float total = 0.f;
            for (int a0 = -1; a0 <= 1; ++a0)
                for (int a1 = -1; a1 <= 1; ++a1)
                    for (int a2 = -1; a2 <= 1; ++a2) {
                        const float e0 = (float)(i0 + a0 - centre) * p.a - Lx[e];
                        const float e1 = (float)(i1 + a1 - centre) * p.a - Ly[e];
                        const float e2 = (float)(i2 + a2 - centre) * p.a - Lz[e];
                        const float r2 = (e0 * e0 + e1 * e1) + e2 * e2;
                        total = total + expf(-(r2 * Lk[e]));
                    }
            Lt[e] = total;
        }
    }
    // The list binned by x-plane: Lp holds the list positions of the atoms whose voxel has i0 == plane, plane after plane, each
    // plane's in list (= atom) order; Ps[plane] is where a plane starts.  Counts by integer LDS atomics (their order does not
    // matter), the fill by one ordered ballot compaction per plane, planes dealt to the four waves.
    for (int q = tid; q <= V; q += 256) Ps[q] = 0;
    __syncthreads();
    for (int e = tid; e < count; e += 256) atomicAdd(&Ps[((Li[e] >> 18) & 511) + 1], 1);
    __syncthreads();
    if (tid == 0)
        for (int q = 0; q < V; ++q) Ps[q + 1] += Ps[q];
    __syncthreads();
    for (int q = wave; q < V; q += 4) {
        int pos = Ps[q];
        for (int base = 0; base < count; base += 64) {
            const int e = base + lane;
            const bool hit = e < count && ((Li[e] >> 18) & 511) == q;
            const unsigned long long m = __ballot(hit);
            if (hit) Lp[pos + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)e;
            pos += __popcll(m);
        }
    }
    __syncthreads();
    const int V3 = V * V * V;
    for (int v = tid; v < V3; v += 256) {
        const int x0 = v / (V * V), rem = v - x0 * V * V, x1 = rem / V, x2 = rem - x1 * V;
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        // A voxel of plane x0 can only receive from atoms of the planes x0 - 1, x0, x0 + 1 (Gaussian) or x0 (boolean).  They are
        // visited in list order, as a walk of the whole list would visit them between the atoms it skips: a three-way merge of the
        // planes' runs by list position.  A wave's voxels lie in one or two planes, so its lanes walk the same runs.
        const int none = 0xFFFF;
        int ca = p.gaussian && x0 > 0 ? Ps[x0 - 1] : 0, ea = p.gaussian && x0 > 0 ? Ps[x0] : 0;
        int cb = Ps[x0], eb = Ps[x0 + 1];
        int cc = p.gaussian && x0 + 1 < V ? Ps[x0 + 1] : 0, ec = p.gaussian && x0 + 1 < V ? Ps[x0 + 2] : 0;
        int ha = ca < ea ? Lp[ca] : none, hb = cb < eb ? Lp[cb] : none, hc = cc < ec ? Lp[cc] : none;
        for (;;) {
            const int e = min(ha, min(hb, hc));
            if (e == none) break;
            if (e == ha) { ++ca; ha = ca < ea ? Lp[ca] : none; }
            else if (e == hb) { ++cb; hb = cb < eb ? Lp[cb] : none; }
            else { ++cc; hc = cc < ec ? Lp[cc] : none; }
            const int pk = Li[e];
            const int i0 = (pk >> 18) & 511, i1 = (pk >> 9) & 511, i2 = pk & 511, ch = (pk >> 27) & 15;
            const int a0 = x0 - i0, a1 = x1 - i1, a2 = x2 - i2;
            if (p.gaussian) {
                if (a0 < -1 || a0 > 1 || a1 < -1 || a1 > 1 || a2 < -1 || a2 > 1) continue;
                const float e0 = (float)(x0 - centre) * p.a - Lx[e];
                const float e1 = (float)(x1 - centre) * p.a - Ly[e];
                const float e2 = (float)(x2 - centre) * p.a - Lz[e];
                const float r2 = (e0 * e0 + e1 * e1) + e2 * e2;
                const float w = expf(-(r2 * Lk[e])) / Lt[e];
                const float ww = Lw[e] * w;                      // rounded to float32, then added
#pragma unroll
                for (int c = 0; c < 8; ++c) if (c == ch) acc[c] = acc[c] + ww;
            } else if ((a0 | a1 | a2) == 0) {
#pragma unroll
                for (int c = 0; c < 8; ++c) if (c == ch) acc[c] = 1.f;
            }
        }
        const size_t o = ((size_t)r * V3 + v) * p.C;
        if (p.gaussian) { for (int c = 0; c < p.C; ++c) ((float*)p.out)[o + c] = acc[c < 8 ? c : 0]; }
        else { for (int c = 0; c < p.C; ++c) ((unsigned char*)p.out)[o + c] = acc[c < 8 ? c : 0] != 0.f ? 1 : 0; }
    }
}

// Creating and destroying a non-blocking stream takes about 3 ms (profiles/voxelise_batch.txt), twice what a whole th_voxelise call
// for one structure took before: a call borrows its stream and hands it back.  Calls that run at the same time hold different
// streams; idle ones are kept for the life of the process (as many as calls ever overlapped).
std::mutex g_idle_mu;
std::vector<std::pair<int, hipStream_t>> g_idle;      // (device, stream)

hipError_t borrow_stream(int device, hipStream_t* st) {
    {
        std::lock_guard<std::mutex> lock(g_idle_mu);
        for (size_t i = 0; i < g_idle.size(); ++i)
            if (g_idle[i].first == device) {
                *st = g_idle[i].second;
                g_idle.erase(g_idle.begin() + i);
                return hipSuccess;
            }
    }
    return hipStreamCreateWithFlags(st, hipStreamNonBlocking);
}

// what one call owns on the device; everything goes when the call returns, whichever way
struct VbCall {
    int device = -1;
    hipStream_t st = nullptr;
    unsigned char* mem = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    ~VbCall() {
        if (device < 0) return;
        (void)hipSetDevice(device);
        if (st) {
            (void)hipStreamSynchronize(st);
            std::lock_guard<std::mutex> lock(g_idle_mu);
            g_idle.emplace_back(device, st);
        }
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (mem) (void)hipFree(mem);
    }
};

// Everything both entry points do; `who` is the entry point's name for th_last_error.  frame_structure may be NULL from th_voxelise
// alone: every frame then belongs to structure 0, and the device array is zeroed in place of an upload.
int voxelise_call(const char* who, int device, const float* atoms_xyz, const int32_t* atom_channel, const float* atom_sigma,
                  const float* atom_weight, int64_t n_atoms, const int64_t* atom_offsets, int64_t n_structures, const float* frames_rt,
                  const int32_t* frame_structure, int64_t n_frames, int voxels_per_side, float frame_edge_length, int n_channels,
                  int gaussian, void* out, int out_on_device, double* kernel_ms) {
    // ---- refusals: all of them before the first HIP call ----
    if (n_atoms < 0 || n_structures < 0 || n_frames < 0)
        TH_FAIL(TH_EINVAL, "%s: negative size (n_atoms = %lld, n_structures = %lld, n_frames = %lld)", who, (long long)n_atoms,
                (long long)n_structures, (long long)n_frames);
    if (n_frames > INT_MAX || n_structures > INT_MAX)
        TH_FAIL(TH_EINVAL, "%s: %lld frames of %lld structures in one call (limit 2^31 - 1 each)", who, (long long)n_frames, (long long)n_structures);
    if (n_atoms && (!atoms_xyz || !atom_channel)) TH_FAIL(TH_EINVAL, "%s: n_atoms = %lld needs atoms_xyz and atom_channel", who, (long long)n_atoms);
    if (gaussian && n_atoms && !atom_sigma) TH_FAIL(TH_EINVAL, "%s: Gaussian frames need per-atom sigmas", who);
    if ((n_atoms || n_structures) && !atom_offsets) TH_FAIL(TH_EINVAL, "%s: atom_offsets is NULL (n_structures + 1 entries)", who);
    if (n_frames && (!frames_rt || !out)) TH_FAIL(TH_EINVAL, "%s: %lld frames need frames_rt and out", who, (long long)n_frames);
    if (atom_offsets)
        if (int rc = th_check_offsets(who, "atom_offsets", "n_atoms", atom_offsets, n_structures, n_atoms)) return rc;
    if (frame_structure)
        for (int64_t r = 0; r < n_frames; ++r)
            if (frame_structure[r] < 0 || frame_structure[r] >= n_structures)
                TH_FAIL(TH_EINVAL, "%s: frame_structure[%lld] = %d is outside [0, %lld)", who, (long long)r, (int)frame_structure[r], (long long)n_structures);
    if (atom_weight && !gaussian) TH_FAIL(TH_EINVAL, "%s: atom_weight with boolean frames (they carry no weight)", who);
    if (atom_weight)
        for (int64_t i = 0; i < n_atoms; ++i)
            if (!std::isfinite(atom_weight[i])) TH_FAIL(TH_EINVAL, "%s: atom_weight[%lld] = %g is not finite", who, (long long)i, (double)atom_weight[i]);
    if (voxels_per_side < 1 || voxels_per_side > 511 || !(voxels_per_side & 1))
        TH_FAIL(TH_EINVAL, "%s: voxels_per_side = %d must be odd and < 512", who, voxels_per_side);
    if (n_channels < 1 || n_channels > 8) TH_FAIL(TH_EUNSUP, "%s: %d channels (1..8)", who, n_channels);
    if (!(frame_edge_length > 0.f)) TH_FAIL(TH_EINVAL, "%s: frame_edge_length = %g is not positive", who, (double)frame_edge_length);
    if (kernel_ms) *kernel_ms = 0.0;
    if (n_frames == 0) return TH_OK;

    VbCall call;
    HIP_TRY(hipSetDevice(device));
    call.device = device;
    const size_t na = (size_t)n_atoms, ns = (size_t)n_structures, nf = (size_t)n_frames;
    const size_t V3 = (size_t)voxels_per_side * voxels_per_side * voxels_per_side;
    const size_t out_bytes = nf * V3 * n_channels * (gaussian ? sizeof(float) : 1);
    ThLayout lay;
    const size_t off_xyz = lay.take(na * 12), off_chn = lay.take(na * 4), off_sig = lay.take(na * 4), off_wgt = lay.take(na * 4);
    const size_t off_offsets = lay.take((ns + 1) * sizeof(int64_t)), off_fs = lay.take(nf * 4), off_frt = lay.take(nf * 48), off_flag = lay.take(4);
    const size_t off_out = lay.take(out_on_device ? 0 : out_bytes);
    if (int rc = th_alloc_or_fail(who, &call.mem, lay.bytes)) return rc;
    HIP_TRY(borrow_stream(device, &call.st));
    if (kernel_ms)
        for (hipEvent_t& ev : call.ev) HIP_TRY(hipEventCreate(&ev));
    hipStream_t st = call.st;
    unsigned char* m = call.mem;
    if (na) {
        HIP_TRY(hipMemcpyAsync(m + off_xyz, atoms_xyz, na * 12, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(m + off_chn, atom_channel, na * 4, hipMemcpyHostToDevice, st));
        if (atom_sigma) HIP_TRY(hipMemcpyAsync(m + off_sig, atom_sigma, na * 4, hipMemcpyHostToDevice, st));
        if (atom_weight) HIP_TRY(hipMemcpyAsync(m + off_wgt, atom_weight, na * 4, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipMemcpyAsync(m + off_offsets, atom_offsets, (ns + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    if (frame_structure) HIP_TRY(hipMemcpyAsync(m + off_fs, frame_structure, nf * 4, hipMemcpyHostToDevice, st));
    else HIP_TRY(hipMemsetAsync(m + off_fs, 0, nf * 4, st));
    HIP_TRY(hipMemcpyAsync(m + off_frt, frames_rt, nf * 48, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(m + off_flag, 0, 4, st));
    void* d_out = out_on_device ? out : (void*)(m + off_out);
    VoxBatchArgs a{(const float*)(m + off_xyz), (const int*)(m + off_chn), (const float*)(m + off_sig), atom_weight ? (const float*)(m + off_wgt) : nullptr,
                   (const long long*)(m + off_offsets), (const int*)(m + off_fs), (const float*)(m + off_frt), voxels_per_side,
                   frame_edge_length / (float)voxels_per_side, n_channels, gaussian, d_out, (int*)(m + off_flag)};
    if (kernel_ms) HIP_TRY(hipEventRecord(call.ev[0], st));
    hipLaunchKernelGGL(k_voxelise_batch, dim3((unsigned)n_frames), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    if (kernel_ms) HIP_TRY(hipEventRecord(call.ev[1], st));
    int flag = 0;
    HIP_TRY(hipMemcpyAsync(&flag, m + off_flag, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (flag) TH_FAIL(TH_EUNSUP, "%s: %d encodable atoms inside one frame (limit %d)", who, flag, kMaxList);
    if (!out_on_device) {
        HIP_TRY(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    if (kernel_ms) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, call.ev[0], call.ev[1]));
        *kernel_ms = ms;
    }
    return TH_OK;
}

}  // namespace

extern "C" int th_voxelise_batch(int device, const float* atoms_xyz, const int32_t* atom_channel, const float* atom_sigma,
                                 const float* atom_weight, int64_t n_atoms, const int64_t* atom_offsets, int64_t n_structures,
                                 const float* frames_rt, const int32_t* frame_structure, int64_t n_frames, int voxels_per_side,
                                 float frame_edge_length, int n_channels, int gaussian, void* out, int out_on_device, double* kernel_ms) {
    if (n_frames > 0 && !frame_structure) TH_FAIL(TH_EINVAL, "th_voxelise_batch: frame_structure is NULL (n_frames = %lld entries)", (long long)n_frames);
    return voxelise_call("th_voxelise_batch", device, atoms_xyz, atom_channel, atom_sigma, atom_weight, n_atoms, atom_offsets, n_structures,
                         frames_rt, frame_structure, n_frames, voxels_per_side, frame_edge_length, n_channels, gaussian, out, out_on_device, kernel_ms);
}

// one structure that owns every atom and every frame, no weights
extern "C" int th_voxelise(int device, const float* atoms_xyz, const int32_t* atom_channel, const float* atom_sigma, int64_t n_atoms,
                           const float* frames_rt, int64_t n_res, int voxels_per_side, float frame_edge_length, int n_channels,
                           int gaussian, void* out, int out_on_device) {
    const int64_t atom_offsets[2] = {0, n_atoms};
    return voxelise_call("th_voxelise", device, atoms_xyz, atom_channel, atom_sigma, nullptr, n_atoms, atom_offsets, 1, frames_rt, nullptr, n_res,
                         voxels_per_side, frame_edge_length, n_channels, gaussian, out, out_on_device, nullptr);
}
