// Fused Conv3D for gfx950: implicit GEMM on the fp32 matrix cores (v_mfma_f32_32x32x2_f32),
// with the Keras block around it folded in:
//     [BN-affine -> act on the input]  ->  Conv3D(any stride, any k, 'same'/'valid')  -> +bias
//     -> [act / BN-affine ...]  ->  [Max/AveragePooling3D 2x2x2]  -> store at a channel offset
// i.e. one launch per "Conv3D -> ELU -> BatchNorm (-> MaxPool)" block of TIMED (reference
// README.md:254) and per "BN -> ReLU -> Conv -> (Concat)" step of a DenseCPD dense layer.
//
// GEMM view (per workgroup):  M = output voxels of a brick (FB whole frames, or ZB z-planes of one
// frame), N = BN output channels, K = taps x Cin.  The brick's *input* voxels (+halo, zero padded =
// Keras 'same') are staged ONCE per Cin-chunk in LDS as [voxel][CS] fp32; every tap then reads the
// same LDS image at a wave-uniform voxel offset, so HBM/L2 sees each activation once per chunk
// instead of k^3 times.  Weights are pre-packed on the host as [nb][chunk][tap][BN][CS] so that a
// chunk's slabs are one linear, coalesced copy into LDS when they are small (BRES = 1); otherwise every
// lane streams its own B fragments L2 -> registers (BRES = 2).  A operands are fetched with ds_read_b128:
//     lane l = (j = l&31, h = l>>5) reads 4 consecutive input channels  c = 8*kk + 4*h + t
//     A[i=j][k=h] = act[voxel(row j)][c],  B[k=h][j] = W[co j][c]   for MFMA t = 0..3
// (the K order inside a chunk is permuted, identically for A and B — a sum does not care).
// fp32 MFMA is an exact fmaf chain (cdna_hip_programming.md §3), so results match a scalar
// fp32 convolution to accumulation-order rounding.
//
// Row order inside a 32-row MFMA tile is chosen so the epilogue never leaves registers:
// for pooled layers rows are grouped 8 pool-mates at a time (row = 8*pooled + mate); in the
// 32x32 C layout (row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)) a lane then holds mates 0-3 or 4-7 of
// 4 pooled voxels, so a 2x2x2 pool is 3 max ops + one cross-half exchange.
// The 16-wide sibling for Cout <= 20, k_conv_n16, is in conv_n16.hip (same argument struct, conv_brick_args.h; no shared device code).
#include "conv_brick_args.h"
#include "device_math.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

#ifndef STAGE_U
#define STAGE_U 8  // staging loads in flight per thread
#endif

// GEO > 0 (streamed 16-channel variants, 3x3x3, stride 1): Hp = Wp = GEO at compile time; see the tap loop.
template <int WAVES, int TM, int TN, int NT, int CI, int BRES, int POOL, int GEO = 0>
__global__ void __launch_bounds__(WAVES * 64, WAVES == 4 ? 2 : 1) k_conv_mfma(const ConvMfmaArgs a) {
    constexpr int NTHREADS = WAVES * 64;
    constexpr int BN = NT * 32;
    constexpr int CI4 = CI / 4;
    constexpr int KK = CI / 8;
    static_assert(NT % TN == 0, "NT must be a multiple of TN");
    extern __shared__ __attribute__((aligned(16))) float4 smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int CS4 = a.CS >> 2;

    // ---- workgroup -> (frame group, z brick, channel block) ---------------------------------
    int bid = blockIdx.x;
    const int nb = bid % a.nnb; bid /= a.nnb;
    const int zb = bid % a.nzb; bid /= a.nzb;
    const int64_t f0 = (int64_t)bid * a.FB;
    const int z0 = zb * a.ZB;

    // ---- LDS carve-up ---------------------------------------------------------------------------
    // GEO kernels: 3x3x3, stride 1, Hp = Wp = GEO and Hc = Wc = GEO - 2, so the table arithmetic divides by constants
    const int gHp = GEO ? GEO : a.Hp, gWp = GEO ? GEO : a.Wp, gHc = GEO ? GEO - 2 : a.Hc, gWc = GEO ? GEO - 2 : a.Wc;
    const int nvox = a.FB * a.Zp * gHp * gWp;
    float4* A4 = smem;
    float4* B4 = A4 + (size_t)nvox * CS4;
    const int bslab4 = BN * CS4;  // one tap's weights
    int* rowvox = (int*)(reinterpret_cast<char*>(smem) + a.tab_off);
    int* rowout = rowvox + a.nrows;
    int* tapoff = rowout + (POOL ? a.nrows / 8 : a.nrows);  // staged-voxel offset of every tap
    for (int t = tid; t < a.ntaps; t += NTHREADS) {
        const int dz = t / (a.kh * a.kw), r2 = t - dz * (a.kh * a.kw), dy = r2 / a.kw, dx = r2 - dy * a.kw;
        tapoff[t] = (dz * gHp + dy) * gWp + dx;
    }
    int* voxsrc = tapoff + a.ntaps;  // staged voxel -> source offset (floats, relative to frame f0) or -1
    for (int v = tid; v < nvox; v += NTHREADS) {
        const int xl = v % gWp; int t = v / gWp;
        const int yl = t % gHp; t /= gHp;
        const int zl = t % a.Zp; const int f = t / a.Zp;
        const int zi = z0 * a.sd + zl - a.pz, yi = yl - a.py, xi = xl - a.px;   // staged plane zl of the brick = input plane z0*sd + zl - pz
        const bool ok = (f0 + f) < a.nframes && zi >= 0 && zi < a.Din && yi >= 0 && yi < a.Hin && xi >= 0 && xi < a.Win;
        voxsrc[v] = ok ? f * (int)a.in_fs + ((zi * a.Hin + yi) * a.Win + xi) * a.in_cs : -1;
    }

    // per m-tile bitmask over dz: set when EVERY row of the tile reads the zero halo for that dz
    int* tskip = voxsrc + nvox;
    for (int mt = tid; mt < a.n_mtiles; mt += NTHREADS) {
        int mask = 0;
        if (POOL == 0 && a.zmajor) {
            const int ZBv = min(a.ZB, a.Dc - z0);
            const int fhw = a.FB * gHc * gWc, total = ZBv * fhw;
            if (mt * 32 >= total) mask = 0xff;
            else {
                const int zlo = z0 + (mt * 32) / fhw, zhi = z0 + min(mt * 32 + 31, total - 1) / fhw;
                for (int dz = 0; dz < a.kd && dz < 8; ++dz)
                    if (zhi + dz - a.pz < 0 || zlo + dz - a.pz >= a.Din) mask |= 1 << dz;
            }
        }
        tskip[mt] = mask;
    }

    // ---- row tables: GEMM row -> staged voxel index, and -> output offset -----------------------
    {
        const int ZBv = min(a.ZB, a.Dc - z0);
        for (int r = tid; r < a.nrows; r += NTHREADS) {
            int f = r / a.rows_pf, q = r - f * a.rows_pf;
            bool fok = (f0 + f) < a.nframes;
            int vox = 0, oo = -1;
            if (POOL == 0) {
                const int hw = gHc * gWc;
                bool rok = q < ZBv * hw;
                if (a.zmajor) {
                    // rows ordered (z, frame, y, x): a 32-row tile then usually lies inside ONE z-plane, and
                    // tiles of the first/last plane can skip the taps that only ever see the zero halo
                    const int fhw = a.FB * hw;
                    rok = r < ZBv * fhw;
                    const int zl0 = r / fhw, rem0 = r - zl0 * fhw;
                    f = rem0 / hw;
                    q = zl0 * hw + (rem0 - f * hw);
                    fok = (f0 + f) < a.nframes;
                }
                if (fok && rok) {
                    const int zl = q / hw, rem = q - zl * hw, y = rem / gWc, x = rem - y * gWc;
                    vox = ((f * a.Zp + zl * a.sd) * gHp + y * a.sh) * gWp + x * a.sw;   // window origin of output voxel (zl, y, x)
                    oo = f * (int)a.out_fs + (((z0 + zl) * a.Ho + y) * a.Wo + x) * a.out_cs;
                }
                rowout[r] = oo;
            } else {
                const int pq = q >> 3, mate = q & 7;
                const int PH = gHc >> 1, PW = gWc >> 1;
                if (fok && pq < (ZBv >> 1) * PH * PW) {
                    const int pzz = pq / (PH * PW), rem = pq - pzz * (PH * PW), pyy = rem / PW, pxx = rem - pyy * PW;
                    const int zl = 2 * pzz + (mate >> 2), y = 2 * pyy + ((mate >> 1) & 1), x = 2 * pxx + (mate & 1);
                    vox = ((f * a.Zp + zl) * gHp + y) * gWp + x;
                    oo = f * (int)a.out_fs + ((((z0 >> 1) + pzz) * a.Ho + pyy) * a.Wo + pxx) * a.out_cs;
                }
                if (mate == 0) rowout[r >> 3] = oo;
            }
            rowvox[r] = vox;
        }
    }

    const int nblocks_n = NT / TN;
    const int total_blocks = ((a.n_mtiles + TM - 1) / TM) * nblocks_n;
    const int rounds = (total_blocks + WAVES - 1) / WAVES;
    const float* wbase = a.wpk + (size_t)nb * a.nchunks * a.ntaps * BN * a.CS;
    const float4* wbase4 = reinterpret_cast<const float4*>(wbase);

    for (int rd = 0; rd < rounds; ++rd) {
        const int blk = rd * WAVES + wave;
        const bool active = blk < total_blocks;
        const int mb = active ? blk / nblocks_n : 0;
        const int nbw = active ? blk - mb * nblocks_n : 0;

        f32x16 acc[TM][TN];
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int tn = 0; tn < TN; ++tn)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[tm][tn][i] = 0.f;

        if (rd == 0) __syncthreads();  // row tables visible
        // a wave's TM m-tiles are interleaved (mb, mb + nmb, ...) so that every wave gets its share of the
        // boundary-plane tiles that skip taps
        const int nmb = (a.n_mtiles + TM - 1) / TM;
        int aidx[TM], bidx[TN], skp[TM];
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) {
            const int mt = a.zmajor ? mb + tm * nmb : mb * TM + tm;
            aidx[tm] = (mt < a.n_mtiles ? rowvox[mt * 32 + j] : 0) * CS4 + h;
            skp[tm] = __builtin_amdgcn_readfirstlane((active && mt < a.n_mtiles) ? tskip[mt] : 0xff);
        }
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) bidx[tn] = ((nbw * TN + tn) * 32 + j) * CS4 + h;

        for (int ch = 0; ch < a.nchunks; ++ch) {
            constexpr bool kLdsEpi = (TM * TN > 2);  // the LDS epilogue clobbers the staging area
            const bool need_a = (kLdsEpi || !(a.nchunks == 1 && rd > 0)) && !((a.dbg & 1) && ch > 0);
            const bool need_b = BRES == 2 ? false : need_a;
            __syncthreads();  // everyone is done reading the previous A image / B slabs
            if (need_a) {
                // ---- stage the haloed input brick for channels [ch*CI, ch*CI+CI) ------------------
                // voxsrc[v] (built once per workgroup) holds the source offset of staged voxel v or -1 for
                // halo / out-of-range: no index arithmetic here, and loads go out 4 at a time so their L2
                // latencies overlap instead of serialising.
                constexpr int U = STAGE_U;
                const int nvec = nvox * CI4;
                const float* inb = a.in + f0 * a.in_fs + a.in_coff + ch * CI;
                const bool has_pre = a.pre.scale || a.pre.act != ACT_LINEAR;
                if (GEO > 0 && a.geo_compact) {
                    // Only voxels that exist are staged from memory: real voxel rr of a frame is input voxel rr, and its
                    // staged position follows from constant divisions.  The halo (42 % of a 12^3 image, 64 % of two 7^3
                    // ones) is zeroed with the first chunk — plain LDS writes, no table lookups, no loads — and nothing
                    // writes it again until an LDS-scratch epilogue.  geo_compact (host): 'same' padding, the whole frame in
                    // one brick, Hin = Win = GEO - 2, float4-aligned full chunks.
                    constexpr int N = GEO - 2;
                    const int per_frame = a.Din * N * N;
                    const int nfv = (int)min((int64_t)a.FB, a.nframes - f0);
                    const int nreal4 = nfv * per_frame * CI4;
                    if (ch == 0) {
                        const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
                        for (int v = tid; v < nvox; v += NTHREADS) {
                            const int x = v % GEO, t = v / GEO, y = t % GEO, t2 = t / GEO, z = t2 % a.Zp, f = t2 / a.Zp;
                            if (x == 0 || x == GEO - 1 || y == 0 || y == GEO - 1 || z == 0 || z == a.Zp - 1 || f >= nfv) {
#pragma unroll
                                for (int g = 0; g < CI4; ++g) A4[(size_t)v * CS4 + g] = zero4;
                            }
                        }
                    }
                    for (int base = tid; base < nreal4; base += NTHREADS * U) {
                        float4 val[U];
                        int dst[U];
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            const int i = min(base + u * NTHREADS, nreal4 - 1);
                            const int r = i / CI4, g = i % CI4;
                            const int f = r / per_frame, rr = r - f * per_frame;
                            const int z = rr / (N * N), y = (rr / N) % N, x = rr % N;
                            dst[u] = (((f * a.Zp + z + 1) * GEO + y + 1) * GEO + x + 1) * CS4 + g;
                            val[u] = *reinterpret_cast<const float4*>(inb + f * a.in_fs + rr * a.in_cs + g * 4);
                        }
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            if (base + u * NTHREADS >= nreal4) continue;
                            if (has_pre) {
                                const int c0 = ch * CI + (dst[u] % CS4) * 4;
                                float e[4] = {val[u].x, val[u].y, val[u].z, val[u].w};
                                if (a.pre.scale) {
#pragma unroll
                                    for (int k = 0; k < 4; ++k) e[k] = fmaf(e[k], a.pre.scale[c0 + k], a.pre.shift[c0 + k]);
                                }
                                th_act_vec<4>(e, a.pre.act, a.pre.alpha);   // decoded once per vector (see device_math.h)
                                val[u] = make_float4(e[0], e[1], e[2], e[3]);
                            }
                            A4[dst[u]] = val[u];
                        }
                    }
                } else
                for (int base = tid; base < nvec; base += NTHREADS * U) {
                    int off[U];
                    float4 val[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int i = base + u * NTHREADS;
                        off[u] = (i < nvec) ? voxsrc[i / CI4] : -1;
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int i = base + u * NTHREADS;
                        const int g = i % CI4;
                        const int c0 = ch * CI + g * 4;
                        val[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (off[u] >= 0 && c0 < a.Cin) {
                            const float* src = inb + off[u] + g * 4;
                            if (a.vec_ok && c0 + 4 <= a.Cin) {
                                val[u] = *reinterpret_cast<const float4*>(src);
                            } else {
                                val[u].x = src[0];
                                if (c0 + 1 < a.Cin) val[u].y = src[1];
                                if (c0 + 2 < a.Cin) val[u].z = src[2];
                                if (c0 + 3 < a.Cin) val[u].w = src[3];
                            }
                        }
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int i = base + u * NTHREADS;
                        if (i >= nvec) continue;
                        const int v = i / CI4, g = i % CI4;
                        if (has_pre && off[u] >= 0) {
                            const int c0 = ch * CI + g * 4;
                            float e[4] = {val[u].x, val[u].y, val[u].z, val[u].w}, y[4];
#pragma unroll
                            for (int k = 0; k < 4; ++k) {
                                const int c = min(c0 + k, a.Cin - 1);
                                y[k] = a.pre.scale ? fmaf(e[k], a.pre.scale[c], a.pre.shift[c]) : e[k];
                            }
                            th_act_vec<4>(y, a.pre.act, a.pre.alpha);   // decoded once per vector (see device_math.h)
#pragma unroll
                            for (int k = 0; k < 4; ++k)
                                if (c0 + k < a.Cin) e[k] = y[k];
                            val[u] = make_float4(e[0], e[1], e[2], e[3]);
                        }
                        A4[(size_t)v * CS4 + g] = val[u];
                    }
                }
            }
            const float4* wch4 = wbase4 + (size_t)ch * a.ntaps * bslab4;
            if (need_b) {
                const int n4 = a.ntaps * bslab4;
                for (int i = tid; i < n4; i += NTHREADS) B4[i] = wch4[i];
            }
            __syncthreads();

            if (BRES == 2) {
                // weights streamed L2 -> registers, one tap ahead: every lane fetches exactly its own MFMA
                // B fragments (host layout [nb][chunk][tap][kk][ntile][lane] float4, 1 KiB per wave-load), so
                // there is no weight slab in LDS and NO barrier inside a Cin-chunk — the 8 waves drift apart
                // and cover each other's LDS latency.
                if (active) {
                    constexpr int TAPSTRIDE = KK * NT * 64;
                    const float4* wf = reinterpret_cast<const float4*>(a.wpk) +
                                       ((size_t)(nb * a.nchunks + ch) * a.ntaps) * TAPSTRIDE + (nbw * TN) * 64 + lane;
                    // Software pipeline, pinned with sched_barrier so hipcc cannot sink the loads back next to
                    // their uses.  Per stage (= 8 input channels of one tap): the NEXT stage's A fragments are
                    // requested from LDS before this stage's TM*TN*4 MFMAs and consumed after them (ping-pong
                    // register sets, no copies); a stage's B fragments are re-loaded for the next tap right
                    // after their last use, so they have a whole stage (>= 2048 MFMA cycles) to arrive from L2.
                    // Tap offsets come from scalar counters: no memory access, no wait, on the address path.
                    int tz = 0, ty = 0, tx = 0;  // coordinates of the NEXT tap
                    auto advance = [&]() {       // returns the staged-voxel offset of the next tap (clamped at the end)
                        if (tx + 1 < a.kw) ++tx;
                        else if (ty + 1 < a.kh) { tx = 0; ++ty; }
                        else if (tz + 1 < a.kd) { tx = 0; ty = 0; ++tz; }
                        return ((tz * a.Hp + ty) * a.Wp + tx) * CS4;
                    };
                    if constexpr (GEO > 0 && KK == 2) {
                        // Compile-time geometry: the nine in-plane taps of a dz plane are unrolled and their staged-voxel
                        // offsets are IMMEDIATES of the ds_read_b128 instructions (relative to a per-dz base), the weight
                        // pointer just advances — no scalar tap counters, no v_add per fragment read.  Every non-MFMA
                        // instruction in this loop delays the next MFMA issue by about its own issue time: on the bare
                        // stage structure (tools/microbench/stage_bench.hip) the address arithmetic costs 2.4 % of the
                        // matrix pipe (151.8 -> 155.4 TFLOP/s).
                        constexpr int C5 = (CI + 4) / 4;          // float4 per staged voxel (CS = CI + 4)
                        constexpr int PLANE = GEO * GEO * C5;     // one dz step
                        float4 bc[2][TN], avA[TM], avB[TM];
#pragma unroll
                        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                            for (int tn = 0; tn < TN; ++tn) bc[kk][tn] = wf[(kk * NT + tn) * 64];
                        int az[TM];
#pragma unroll
                        for (int tm = 0; tm < TM; ++tm) { az[tm] = aidx[tm]; avA[tm] = A4[az[tm]]; }
                        const float4* wt = wf;   // the current tap's fragments
                        for (int dz = 0; dz < 3; ++dz) {
                            const int nxt_plane = dz < 2 ? PLANE : (2 * GEO + 2) * C5;   // after the last tap: re-read it
#pragma unroll
                            for (int t9 = 0; t9 < 9; ++t9) {
                                const int cur = ((t9 / 3) * GEO + t9 % 3) * C5;
                                const int nxt = (((t9 + 1) / 3) * GEO + (t9 + 1) % 3) * C5;
                                const float4* wn = (t9 == 8 && dz == 2) ? wt : wt + TAPSTRIDE;
                                // ---- stage 0 ----
#pragma unroll
                                for (int tm = 0; tm < TM; ++tm) avB[tm] = A4[az[tm] + cur + 2];
                                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                                for (int tm = 0; tm < TM; ++tm) {
                                    if ((skp[tm] >> dz) & 1) continue;  // whole tile sees only the zero halo for this dz
#pragma unroll
                                    for (int tn = 0; tn < TN; ++tn) {
                                        acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(avA[tm].x, bc[0][tn].x, acc[tm][tn], 0, 0, 0);
                                        acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(avA[tm].y, bc[0][tn].y, acc[tm][tn], 0, 0, 0);
                                        acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(avA[tm].z, bc[0][tn].z, acc[tm][tn], 0, 0, 0);
                                        acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(avA[tm].w, bc[0][tn].w, acc[tm][tn], 0, 0, 0);
                                    }
                                }
                                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                                for (int tn = 0; tn < TN; ++tn) bc[0][tn] = wn[tn * 64];
                                // ---- stage 1 ----
#pragma unroll
                                for (int tm = 0; tm < TM; ++tm) avA[tm] = A4[az[tm] + (t9 < 8 ? nxt : nxt_plane)];
                                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                                for (int tm = 0; tm < TM; ++tm) {
                                    if ((skp[tm] >> dz) & 1) continue;
#pragma unroll
                                    for (int tn = 0; tn < TN; ++tn) {
                                        acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(avB[tm].x, bc[1][tn].x, acc[tm][tn], 0, 0, 0);
                                        acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(avB[tm].y, bc[1][tn].y, acc[tm][tn], 0, 0, 0);
                                        acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(avB[tm].z, bc[1][tn].z, acc[tm][tn], 0, 0, 0);
                                        acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(avB[tm].w, bc[1][tn].w, acc[tm][tn], 0, 0, 0);
                                    }
                                }
                                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                                for (int tn = 0; tn < TN; ++tn) bc[1][tn] = wn[(NT + tn) * 64];
                                wt = wn;
                            }
#pragma unroll
                            for (int tm = 0; tm < TM; ++tm) az[tm] += PLANE;
                        }
                    } else if (KK == 2) {
                        float4 bc[2][TN], avA[TM], avB[TM];
#pragma unroll
                        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                            for (int tn = 0; tn < TN; ++tn) bc[kk][tn] = wf[(kk * NT + tn) * 64];
#pragma unroll
                        for (int tm = 0; tm < TM; ++tm) avA[tm] = A4[aidx[tm]];
                        int toff_cur = 0;
                        for (int tap = 0; tap < a.ntaps; ++tap) {
                            const int cz = tz;  // dz of the current tap
                            const int toff_nxt = advance();
                            const float4* wn = wf + (size_t)min(tap + 1, a.ntaps - 1) * TAPSTRIDE;
                            // ---- stage 0 ----
#pragma unroll
                            for (int tm = 0; tm < TM; ++tm) avB[tm] = A4[aidx[tm] + toff_cur + 2];
                            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                            for (int tm = 0; tm < TM; ++tm) {
                                if (__builtin_expect((skp[tm] >> cz) & 1, 0)) continue;  // whole tile sees only the zero halo for this dz
#pragma unroll
                                for (int tn = 0; tn < TN; ++tn) {
                                    acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(avA[tm].x, bc[0][tn].x, acc[tm][tn], 0, 0, 0);
                                    acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(avA[tm].y, bc[0][tn].y, acc[tm][tn], 0, 0, 0);
                                    acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(avA[tm].z, bc[0][tn].z, acc[tm][tn], 0, 0, 0);
                                    acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(avA[tm].w, bc[0][tn].w, acc[tm][tn], 0, 0, 0);
                                }
                            }
                            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                            for (int tn = 0; tn < TN; ++tn) bc[0][tn] = wn[tn * 64];
                            // ---- stage 1 ----
#pragma unroll
                            for (int tm = 0; tm < TM; ++tm) avA[tm] = A4[aidx[tm] + toff_nxt];
                            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                            for (int tm = 0; tm < TM; ++tm) {
                                if (__builtin_expect((skp[tm] >> cz) & 1, 0)) continue;  // whole tile sees only the zero halo for this dz
#pragma unroll
                                for (int tn = 0; tn < TN; ++tn) {
                                    acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(avB[tm].x, bc[1][tn].x, acc[tm][tn], 0, 0, 0);
                                    acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(avB[tm].y, bc[1][tn].y, acc[tm][tn], 0, 0, 0);
                                    acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(avB[tm].z, bc[1][tn].z, acc[tm][tn], 0, 0, 0);
                                    acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(avB[tm].w, bc[1][tn].w, acc[tm][tn], 0, 0, 0);
                                }
                            }
                            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                            for (int tn = 0; tn < TN; ++tn) bc[1][tn] = wn[(NT + tn) * 64];
                            toff_cur = toff_nxt;
                        }
                    } else {
                        float4 bcur[KK][TN], bnxt[KK][TN], av[TM], avn[TM];
#pragma unroll
                        for (int kk = 0; kk < KK; ++kk)
#pragma unroll
                            for (int tn = 0; tn < TN; ++tn) bcur[kk][tn] = wf[(kk * NT + tn) * 64];
#pragma unroll
                        for (int tm = 0; tm < TM; ++tm) av[tm] = A4[aidx[tm]];
                        int toff_cur = 0;
                        for (int tap = 0; tap < a.ntaps; ++tap) {
                            const int toff_nxt = advance();
                            const float4* wn = wf + (size_t)min(tap + 1, a.ntaps - 1) * TAPSTRIDE;
#pragma unroll
                            for (int kk = 0; kk < KK; ++kk)
#pragma unroll
                                for (int tn = 0; tn < TN; ++tn) bnxt[kk][tn] = wn[(kk * NT + tn) * 64];
#pragma unroll
                            for (int kk = 0; kk < KK; ++kk) {
                                const int noff = (kk + 1 < KK) ? toff_cur + (kk + 1) * 2 : toff_nxt;
#pragma unroll
                                for (int tm = 0; tm < TM; ++tm) avn[tm] = A4[aidx[tm] + noff];
                                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                                for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                                    for (int tn = 0; tn < TN; ++tn) {
                                        acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[tm].x, bcur[kk][tn].x, acc[tm][tn], 0, 0, 0);
                                        acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[tm].y, bcur[kk][tn].y, acc[tm][tn], 0, 0, 0);
                                        acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[tm].z, bcur[kk][tn].z, acc[tm][tn], 0, 0, 0);
                                        acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[tm].w, bcur[kk][tn].w, acc[tm][tn], 0, 0, 0);
                                    }
                                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                                for (int tm = 0; tm < TM; ++tm) av[tm] = avn[tm];
                            }
#pragma unroll
                            for (int kk = 0; kk < KK; ++kk)
#pragma unroll
                                for (int tn = 0; tn < TN; ++tn) bcur[kk][tn] = bnxt[kk][tn];
                            toff_cur = toff_nxt;
                        }
                    }
                }
            } else {   // BRES == 1: every tap's slab is resident in LDS
                if (active) {
                    int tap = 0;
                    for (int dz = 0; dz < a.kd; ++dz)
                        for (int dy = 0; dy < a.kh; ++dy)
                            for (int dx = 0; dx < a.kw; ++dx, ++tap) {
                                const int toff = ((dz * a.Hp + dy) * a.Wp + dx) * CS4;
                                const float4* Bt = B4 + (size_t)tap * bslab4;
#pragma unroll
                                for (int kk = 0; kk < KK; ++kk) {
                                    float4 av[TM], bv[TN];
#pragma unroll
                                    for (int tm = 0; tm < TM; ++tm) av[tm] = A4[aidx[tm] + toff + kk * 2];
#pragma unroll
                                    for (int tn = 0; tn < TN; ++tn) bv[tn] = Bt[bidx[tn] + kk * 2];
#pragma unroll
                                    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                                        for (int tn = 0; tn < TN; ++tn) {
                                            acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[tm].x, bv[tn].x, acc[tm][tn], 0, 0, 0);
                                            acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[tm].y, bv[tn].y, acc[tm][tn], 0, 0, 0);
                                            acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[tm].z, bv[tn].z, acc[tm][tn], 0, 0, 0);
                                            acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[tm].w, bv[tn].w, acc[tm][tn], 0, 0, 0);
                                        }
                                }
                            }
                }
            }
        }  // chunks

        // ---- epilogue: bias, activation / BN-affine chain, optional 2x2x2 pool, store ------------
        constexpr bool REG_EPI = (TM * TN <= 2);
        if (REG_EPI) {
            // small per-wave tiles: finish in registers.  In the 32x32 C layout a lane holds rows
            // (i&3) + 8*(i>>2) + 4*h, i.e. pool-mates 0-3 (h=0) or 4-7 (h=1) of 4 pooled voxels.
            if (active) {
                float* outb = a.out + f0 * a.out_fs + a.out_coff;
#pragma unroll
                for (int tm = 0; tm < TM; ++tm) {
                    const int mt = a.zmajor ? mb + tm * nmb : mb * TM + tm;
                    const bool mt_ok = mt < a.n_mtiles;
#pragma unroll
                    for (int tn = 0; tn < TN; ++tn) {
                        const int co = nb * BN + (nbw * TN + tn) * 32 + j;
                        const bool cok = co < a.Cout && mt_ok;
                        const int cc = co < a.Cout ? co : 0;
                        const float bv = a.bias ? a.bias[cc] : 0.f;
                        float x[16];
#pragma unroll
                        for (int i = 0; i < 16; ++i) x[i] = acc[tm][tn][i] + bv;
                        th_post16(x, cc, a.post);
                        if (POOL == 0) {
#pragma unroll
                            for (int i = 0; i < 16; ++i) {
                                const int oo = cok ? rowout[mt * 32 + (i & 3) + 8 * (i >> 2) + 4 * h] : -1;
                                if (oo >= 0) outb[oo + co] = x[i];
                            }
                        } else {
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                float m;
                                if (POOL == 1) m = fmaxf(fmaxf(x[4 * q], x[4 * q + 1]), fmaxf(x[4 * q + 2], x[4 * q + 3]));
                                else m = (x[4 * q] + x[4 * q + 1]) + (x[4 * q + 2] + x[4 * q + 3]);
                                const float o2 = __shfl_xor(m, 32);
                                m = (POOL == 1) ? fmaxf(m, o2) : (m + o2) * 0.125f;
                                const int oo = cok ? rowout[mt * 4 + q] : -1;
                                if (oo >= 0 && (q >> 1) == h) outb[oo + co] = m;
                            }
                        }
                    }
                }
            }
        } else {
            // big per-wave tiles.  Max-pool in front of a monotone chain (TIMED block 2) needs no scratch at all:
            // a lane holds pool-mates 0-3 (h = 0) or 4-7 (h = 1) of 4 pooled voxels, so 3 max + one cross-half
            // exchange per voxel leave the pooled sums in registers, and the chain runs on 2 values per tile —
            // no LDS round trip, no workgroup barrier in front of the epilogue.
            const bool reg_pool = POOL == 1 && a.post.monotone;
            if (reg_pool) {
                if (active) {
                    float* outb = a.out + f0 * a.out_fs + a.out_coff;
#pragma unroll
                    for (int tm = 0; tm < TM; ++tm) {
                        const int mt = a.zmajor ? mb + tm * nmb : mb * TM + tm;
#pragma unroll
                        for (int tn = 0; tn < TN; ++tn) {
                            const int co = nb * BN + (nbw * TN + tn) * 32 + j;
                            const bool cok = co < a.Cout && mt < a.n_mtiles;
                            const int cc = co < a.Cout ? co : 0;
                            const float bv = a.bias ? a.bias[cc] : 0.f;
                            float m[4];
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                const float mq = fmaxf(fmaxf(acc[tm][tn][4 * q], acc[tm][tn][4 * q + 1]), fmaxf(acc[tm][tn][4 * q + 2], acc[tm][tn][4 * q + 3]));
                                m[q] = fmaxf(mq, __shfl_xor(mq, 32));
                            }
                            // lane half h finishes pooled voxels 2h and 2h + 1 (max commutes with the bias add bit for bit)
                            float v0 = (h ? m[2] : m[0]) + bv, v1 = (h ? m[3] : m[1]) + bv;
                            th_post2(v0, v1, cc, a.post);
                            const int o0 = cok ? rowout[mt * 4 + 2 * h] : -1, o1 = cok ? rowout[mt * 4 + 2 * h + 1] : -1;
                            if (o0 >= 0) outb[o0 + co] = v0;
                            if (o1 >= 0) outb[o1 + co] = v1;
                        }
                    }
                }
            } else {
            // otherwise each 32x32 accumulator tile goes registers -> a per-wave LDS scratch
            // tile -> a compact runtime loop (keeps the activation switch out of a 128-way unroll, so
            // the accumulators stay in VGPRs).  The scratch aliases the A/B staging area (hence the
            // barrier, and hence A is re-staged every round in this mode).
            __syncthreads();
            if (active) {
                float* outb = a.out + f0 * a.out_fs + a.out_coff;
                float* T = reinterpret_cast<float*>(smem) + wave * (32 * 33);
#pragma unroll
                for (int tm = 0; tm < TM; ++tm) {
#pragma unroll
                    for (int tn = 0; tn < TN; ++tn) {
                        const int mt = a.zmajor ? mb + tm * nmb : mb * TM + tm;
#pragma unroll
                        for (int i = 0; i < 16; ++i) T[((i & 3) + 8 * (i >> 2) + 4 * h) * 33 + j] = acc[tm][tn][i];
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                        const int co = nb * BN + (nbw * TN + tn) * 32 + j;
                        const bool cok = co < a.Cout && mt < a.n_mtiles;
                        const int cc = co < a.Cout ? co : 0;
                        const float bv = a.bias ? a.bias[cc] : 0.f;
                        if (POOL == 0) {
                            // lane (j, h) finishes rows h, h+2, ..., h+30 of column j
                            float x[16];
#pragma unroll
                            for (int k = 0; k < 16; ++k) x[k] = T[(2 * k + h) * 33 + j] + bv;
                            th_post16(x, cc, a.post);
#pragma unroll
                            for (int k = 0; k < 16; ++k) {
                                const int oo = cok ? rowout[mt * 32 + 2 * k + h] : -1;
                                if (oo >= 0) outb[oo + co] = x[k];
                            }
                        } else {
                            // lane (j, h) finishes pooled voxels q = h and h+2: their 8 mates each
                            float x[16];
#pragma unroll
                            for (int k = 0; k < 2; ++k)
#pragma unroll
                                for (int e = 0; e < 8; ++e) x[8 * k + e] = T[(8 * (2 * k + h) + e) * 33 + j] + bv;
                            if (POOL == 1 && a.post.monotone) {
                                // max-pool first, then the (monotone non-decreasing) chain on the two pooled values only
                                float m0 = x[0], m1 = x[8];
#pragma unroll
                                for (int e = 1; e < 8; ++e) { m0 = fmaxf(m0, x[e]); m1 = fmaxf(m1, x[8 + e]); }
                                th_post2(m0, m1, cc, a.post);
                                const int o0 = cok ? rowout[mt * 4 + h] : -1, o1 = cok ? rowout[mt * 4 + 2 + h] : -1;
                                if (o0 >= 0) outb[o0 + co] = m0;
                                if (o1 >= 0) outb[o1 + co] = m1;
                            } else {
                                th_post16(x, cc, a.post);
#pragma unroll
                                for (int k = 0; k < 2; ++k) {
                                    float m = x[8 * k];
#pragma unroll
                                    for (int e = 1; e < 8; ++e) m = (POOL == 1) ? fmaxf(m, x[8 * k + e]) : m + x[8 * k + e];
                                    if (POOL == 2) m *= 0.125f;
                                    const int oo = cok ? rowout[mt * 4 + 2 * k + h] : -1;
                                    if (oo >= 0) outb[oo + co] = m;
                                }
                            }
                        }
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                    }
                }
            }
            }
        }
    }  // rounds
}

// ---- tile configurations ------------------------------------------------------------------------
typedef void (*ConvKernel)(const ConvMfmaArgs);
// BRES: 1 all taps' weights resident in LDS, 2 streamed L2 -> registers; k: the instantiation per pool mode
struct CfgDesc { int WAVES, TM, TN, NT, CI, BRES; ConvKernel k[3]; };
#define CFG(W, TM, TN, NT, CI, BR) \
    { W, TM, TN, NT, CI, BR, { k_conv_mfma<W, TM, TN, NT, CI, BR, 0>, k_conv_mfma<W, TM, TN, NT, CI, BR, 1>, k_conv_mfma<W, TM, TN, NT, CI, BR, 2> } }
// kS<waves>N<columns>: 16 input channels per chunk, weights streamed; the three widths of a group in the order 64, 128, 32
enum Cfg : int { kC8Res32, kC8Res64, kS8N64, kS8N128, kS8N32, kS4N64, kS4N128, kS4N32, kC8Str32, kC8Str64, kS4N96, kNumCfgs };
const CfgDesc kCfgs[kNumCfgs] = {
    CFG(8, 1, 1, 1, 8, 1),   // kC8Res32: Cin<=8, Cout<=32  (first layer: everything resident, many rounds)
    CFG(8, 2, 2, 2, 8, 1),   // kC8Res64: Cin<=8, BN=64
    CFG(8, 4, 2, 2, 16, 2),  // kS8N64:  BN=64,  weights streamed L2 -> registers
    CFG(8, 4, 2, 4, 16, 2),  // kS8N128: BN=128, streamed
    CFG(8, 2, 1, 1, 16, 2),  // kS8N32:  BN=32,  streamed
    CFG(4, 4, 2, 2, 16, 2),  // kS4N64:  4-wave workgroups (two per CU: one's staging hides under the other's MFMAs)
    CFG(4, 4, 2, 4, 16, 2),  // kS4N128
    CFG(4, 2, 1, 1, 16, 2),  // kS4N32
    CFG(8, 2, 1, 1, 8, 2),   // kC8Str32: Cin<=8 with weights streamed (large kernels on the input, e.g. 5^3: 125 taps do not fit LDS)
    CFG(8, 2, 2, 2, 8, 2),   // kC8Str64: same, BN=64
    CFG(4, 2, 3, 3, 16, 2),  // kS4N96:  BN=96 — the last Cout block of a wide layer (338 = 128 + 128 + 82: 352 columns instead of 384)
};

// compile-time staged row geometry (Hp = Wp) for the TIMED layers after the first: 3x3x3, stride 1
struct MfmaGeo { int cfg, pool, geo; ConvKernel k; };
const MfmaGeo kMfmaGeo[] = {
    {kS4N128, 0, 7, k_conv_mfma<4, 4, 2, 4, 16, 2, 0, 7>},    // 5^3 volumes, two frames per workgroup
    {kS8N64, 1, 12, k_conv_mfma<8, 4, 2, 2, 16, 2, 1, 12>},   // 10^3 + 2^3 max-pool
    {kS4N96, 0, 7, k_conv_mfma<4, 2, 3, 3, 16, 2, 0, 7>},     // 5^3, 96-column tail block
    {kS4N64, 0, 7, k_conv_mfma<4, 4, 2, 2, 16, 2, 0, 7>},     // 5^3, 64-column tail block
};

// the full instantiation, as rocprofv3 prints it: what the plan label and th_conv_brick_kernels name
std::string mfma_kernel_name(const CfgDesc& c, int pool, int geo) {
    char buf[64];
    snprintf(buf, sizeof buf, "k_conv_mfma<%d,%d,%d,%d,%d,%d,%d,%d>", c.WAVES, c.TM, c.TN, c.NT, c.CI, c.BRES, pool, geo);
    return buf;
}

}  // namespace

static bool plan_with_cfg(int cfg, size_t lds_limit, bool whole_frames_only, const TView& in, const TView& oc,
                          const ConvGeom& g, int Cin, int Cout, int pool, const ThKnobs& kn, ConvMfmaPlan* p) {
    const CfgDesc& c = kCfgs[cfg];
    p->knobs = &kn;
    p->cfg = cfg;
    p->CI = c.CI;
    p->CS = c.CI == 8 ? 8 : c.CI + 4;  // CI=8: unpadded (2-way ds_read_b128 conflict, but the brick fits)
    p->BN = c.NT * 32;
    p->nnb = (Cout + p->BN - 1) / p->BN;
    p->nchunks = (Cin + c.CI - 1) / c.CI;
    p->pool = pool;
    p->Dc = pool ? (oc.D / 2) * 2 : oc.D;
    p->Hc = pool ? (oc.H / 2) * 2 : oc.H;
    p->Wc = pool ? (oc.W / 2) * 2 : oc.W;
    p->Hp = (p->Hc - 1) * g.sh + g.kh;   // staged (haloed) extent: windows of Hc outputs at stride sh
    p->Wp = (p->Wc - 1) * g.sw + g.kw;
    const int ntaps = g.kd * g.kh * g.kw;
    const size_t bbytes = c.BRES == 2 ? 0 : (size_t)ntaps * p->BN * p->CS * 4;
    auto rows_for = [&](int zb) {
        const int r = pool ? 8 * ((zb / 2) * (p->Hc / 2) * (p->Wc / 2)) : zb * p->Hc * p->Wc;
        return round_up(r, 32);
    };
    auto tab_bytes = [&](int fb, int zb) {
        const size_t nvox = (size_t)fb * ((zb - 1) * g.sd + g.kd) * p->Hp * p->Wp;
        const int nrows = fb * rows_for(zb);
        return (size_t)nrows * 4 + (size_t)(pool ? nrows / 8 : nrows) * 4 + (size_t)ntaps * 4 + nvox * 4 + (size_t)(nrows / 32) * 4;
    };
    auto lds_for = [&](int fb, int zb) {
        const size_t nvox = (size_t)fb * ((zb - 1) * g.sd + g.kd) * p->Hp * p->Wp;
        return std::max(nvox * p->CS * 4 + bbytes, (size_t)c.WAVES * 32 * 33 * 4) + tab_bytes(fb, zb);
    };
    const int max_mt = c.WAVES * c.TM * c.TN / c.NT;  // m-tiles one round covers
    int FB = 0, ZB = 0;
    if (lds_for(1, p->Dc) <= lds_limit && (p->nchunks == 1 || rows_for(p->Dc) / 32 <= max_mt || !whole_frames_only)) {
        ZB = p->Dc;
        FB = 1;
        while (FB < 16 && lds_for(FB + 1, ZB) <= lds_limit &&
               (p->nchunks == 1 || (FB + 1) * rows_for(ZB) / 32 <= max_mt))
            ++FB;
    } else {
        if (whole_frames_only) return false;
        FB = 1;
        const int step = pool ? 2 : 1;
        for (int zb = p->Dc - step; zb >= step; zb -= step)
            if (lds_for(1, zb) <= lds_limit) { ZB = zb; break; }
        if (ZB == 0) return false;
        // prefer a brick height that divides the extent evenly if one exists at >= 60% of the max
        for (int zb = ZB; zb >= step && zb * 10 >= ZB * 6; zb -= step)
            if (p->Dc % zb == 0) { ZB = zb; break; }
    }
    p->FB = FB;
    p->ZB = ZB;
    p->nzb = (p->Dc + ZB - 1) / ZB;
    p->Zp = (ZB - 1) * g.sd + g.kd;
    p->rows_pf = rows_for(ZB);
    p->lds_bytes = lds_for(FB, ZB);
    p->tab_off = p->lds_bytes - tab_bytes(FB, ZB);
    p->wpk_floats = (size_t)p->nnb * p->nchunks * ntaps * p->BN * (c.BRES == 2 ? c.CI : p->CS);
    const double rows_exec = (double)p->nzb * p->rows_pf;  // per frame
    p->exec_flops = 2.0 * rows_exec * (double)(p->nnb * p->BN) * (double)(p->nchunks * c.CI) * ntaps;
    if (p->pool == 0 && c.BRES == 2 && c.CI == 16 && g.kd <= 8 && g.sd == 1 && g.sh == 1 && g.sw == 1) {
        // z-major rows: m-tiles whose rows all read the zero halo for a dz skip that dz's taps
        // (same rule as the kernel's tskip table); exec_flops counts what is actually issued
        const int n_mtiles = FB * p->rows_pf / 32, fhw = FB * p->Hc * p->Wc;
        double issued = 0, full = 0;
        for (int zbk = 0; zbk < p->nzb; ++zbk) {
            const int z0 = zbk * ZB, ZBv = std::min(ZB, p->Dc - z0), total = ZBv * fhw;
            for (int mt = 0; mt < n_mtiles; ++mt) {
                full += g.kd;
                if (mt * 32 >= total) continue;   // whole tile is padding: never issued
                const int zlo = z0 + (mt * 32) / fhw, zhi = z0 + std::min(mt * 32 + 31, total - 1) / fhw;
                for (int dz = 0; dz < g.kd; ++dz)
                    if (!(zhi + dz - g.pz < 0 || zlo + dz - g.pz >= in.D)) issued += 1;
            }
        }
        if (full > 0) p->exec_flops *= issued / full;
    }
    if ((int64_t)FB * oc.fs > 0x7fffffffLL || (int64_t)FB * in.D * in.H * in.W * std::max(in.cs, in.C) > 0x7fffffffLL) return false;
    p->geo = 0;
    if (g.kd == 3 && g.kh == 3 && g.kw == 3 && g.sd == 1 && g.sh == 1 && g.sw == 1 && p->Hp == p->Wp && p->CS == 20)
        for (const MfmaGeo& ge : kMfmaGeo)
            if (ge.cfg == cfg && ge.pool == pool && ge.geo == p->Hp) p->geo = ge.geo;
    char buf[224];
    snprintf(buf, sizeof buf, "conv_mfma<w%d,%dx%d,nt%d,ci%d,%s,pool%d> FB%d ZB%d/%d rows%d lds%zuK [%s]",
             c.WAVES, c.TM, c.TN, c.NT, c.CI, c.BRES == 2 ? "stream" : "res", pool, FB, ZB, p->Dc, p->rows_pf,
             p->lds_bytes / 1024, mfma_kernel_name(c, pool, p->geo).c_str());
    p->label = buf;
    return true;
}

// every compiled instantiation, one name per line: kCfgs x pool, then kMfmaGeo
void conv_mfma_kernel_names(std::string* out) {
    for (const CfgDesc& c : kCfgs)
        for (int pool = 0; pool < 3; ++pool) *out += mfma_kernel_name(c, pool, 0) + "\n";
    for (const MfmaGeo& ge : kMfmaGeo) *out += mfma_kernel_name(kCfgs[ge.cfg], ge.pool, ge.geo) + "\n";
}

// the label of a layer whose last Cout block runs on `tail` (conv_mfma_plan_tail); `main` as conv_mfma_plan left it
std::string conv_mfma_tailed_label(const ConvMfmaPlan& main, const ConvMfmaPlan& tail) {
    return main.label + " x" + std::to_string(main.nnb - 1) + " + " + tail.label;
}


bool conv_mfma_plan(const TView& in, const TView& oc, const ConvGeom& g, int Cin, int Cout, int pool, const ThKnobs& kn, ConvMfmaPlan* p) {
    if (g.dd != 1 || g.dh != 1 || g.dw != 1) return false;
    const bool strided = g.sd != 1 || g.sh != 1 || g.sw != 1;
    if (strided && pool) return false;   // strided convolutions run on the brick kernel (row table carries the stride), unpooled
    if (pool && (oc.D < 2 || oc.H < 2 || oc.W < 2)) return false;
    if (Cin <= 8 && Cout <= 64) {
        // weights resident in LDS; a kernel too large for that (5^3: 125 taps) streams them
        const bool n32 = Cout <= 32;
        return plan_with_cfg(n32 ? kC8Res32 : kC8Res64, kLdsLimit, false, in, oc, g, Cin, Cout, pool, kn, p) ||
               plan_with_cfg(n32 ? kC8Str32 : kC8Str64, kLdsLimit, false, in, oc, g, Cin, Cout, pool, kn, p);
    }
    // weights streamed L2 -> registers: two 4-wave workgroups per CU when whole frames fit in half the LDS, else one 8-wave workgroup
    const int width = Cout <= 32 ? 2 : (Cout <= 64 ? 0 : 1);
    return plan_with_cfg(kS4N64 + width, kLdsLimit / 2, true, in, oc, g, Cin, Cout, pool, kn, p) ||
           plan_with_cfg(kS8N64 + width, kLdsLimit, false, in, oc, g, Cin, Cout, pool, kn, p);
}

// Heterogeneous Cout blocks: a layer planned on the two-per-CU 128-column kernel (kS4N128) whose LAST block would be mostly
// zero columns gets that block from a narrower instantiation instead — 96 (kS4N96), 64 (kS4N64) or 32 (kS4N32) columns —
// launched right after the 128-column blocks on the same input.  Every block stages the input once either way (a block
// is a workgroup), so unlike a split over different kernels nothing is staged more often than before.  TIMED-rotamer's
// head (256 -> 338 at 5^3, half of that model's time): 128 + 128 + 96 = 352 columns instead of 3 x 128 = 384.
bool conv_mfma_plan_tail(const TView& in, const TView& oc, const ConvGeom& g, int Cin, int Cout, int pool, const ConvMfmaPlan& main,
                         const ThKnobs& kn, ConvMfmaPlan* tail, int* cout_main) {
    const bool off = kn.conv_notail != 0;     // A/B comparisons and tests
    if (off || main.cfg != kS4N128 || main.nnb < 2) return false;
    const int done = (main.nnb - 1) * main.BN, rest = Cout - done;
    if (rest <= 0 || rest > 96) return false;
    const int cfg = rest <= 32 ? kS4N32 : (rest <= 64 ? kS4N64 : kS4N96);
    if (!plan_with_cfg(cfg, kLdsLimit / 2, true, in, oc, g, Cin, rest, pool, kn, tail)) return false;
    if (tail->nnb != 1) return false;
    *cout_main = done;
    return true;
}

void conv_mfma_pack_weights(const ConvMfmaPlan& p, const ConvGeom& g, int Cin, int Cout, const float* w, float* dst) {
    const int ntaps = g.kd * g.kh * g.kw;
    std::memset(dst, 0, p.wpk_floats * sizeof(float));
    if (kCfgs[p.cfg].BRES == 2) {
        // fragment order: [nb][chunk][tap][kk][ntile][h][j][t]  with  ci = chunk*CI + kk*8 + 4h + t,  co = nb*BN + ntile*32 + j
        const int KK = p.CI / 8, NT = p.BN / 32;
        for (int nb = 0; nb < p.nnb; ++nb)
            for (int ch = 0; ch < p.nchunks; ++ch)
                for (int t = 0; t < ntaps; ++t)
                    for (int kk = 0; kk < KK; ++kk)
                        for (int nt = 0; nt < NT; ++nt) {
                            float* frag = dst + ((((size_t)(nb * p.nchunks + ch) * ntaps + t) * KK + kk) * NT + nt) * 256;
                            for (int h = 0; h < 2; ++h)
                                for (int j = 0; j < 32; ++j) {
                                    const int co = nb * p.BN + nt * 32 + j;
                                    if (co >= Cout) continue;
                                    for (int q = 0; q < 4; ++q) {
                                        const int ci = ch * p.CI + kk * 8 + 4 * h + q;
                                        if (ci < Cin) frag[(h * 32 + j) * 4 + q] = w[((size_t)t * Cin + ci) * Cout + co];
                                    }
                                }
                        }
        return;
    }
    for (int nb = 0; nb < p.nnb; ++nb)
        for (int ch = 0; ch < p.nchunks; ++ch)
            for (int t = 0; t < ntaps; ++t) {
                float* slab = dst + (((size_t)nb * p.nchunks + ch) * ntaps + t) * p.BN * p.CS;
                for (int n = 0; n < p.BN; ++n) {
                    const int co = nb * p.BN + n;
                    if (co >= Cout) break;
                    for (int c = 0; c < p.CI; ++c) {
                        const int ci = ch * p.CI + c;
                        if (ci >= Cin) break;
                        slab[(size_t)n * p.CS + c] = w[((size_t)t * Cin + ci) * Cout + co];
                    }
                }
            }
}

int launch_conv_mfma(hipStream_t s, int64_t n, const ConvMfmaPlan& p, TView in, TView out, ConvGeom g, int Cin, int Cout,
                     const float* wpk, const float* bias, PreOp pre, PostOps post) {
    if (p.cfg < 0 || p.cfg >= kNumCfgs) TH_FAIL(TH_EINVAL, "conv_mfma: bad plan");
    const CfgDesc& c = kCfgs[p.cfg];
    ConvMfmaArgs a = brick_args(p, n, in, out, g, Cin, Cout, wpk, bias, pre, post);
    a.n_mtiles = a.nrows / 32; a.CS = p.CS; a.nnb = p.nnb; a.tab_off = (int)p.tab_off;
    a.zmajor = (p.pool == 0 && c.BRES == 2 && c.CI == 16 && g.sd == 1 && g.sh == 1 && g.sw == 1) ? 1 : 0;
    const int64_t grid = (n + p.FB - 1) / p.FB * p.nzb * p.nnb;
    if (grid > 0x7fffffffLL) TH_FAIL(TH_EINVAL, "conv_mfma: grid too large");
    ConvKernel k = c.k[p.pool];
    if (p.geo)
        for (const MfmaGeo& ge : kMfmaGeo)
            if (ge.cfg == p.cfg && ge.pool == p.pool && ge.geo == p.geo) {
                k = ge.k;
                a.geo_compact = (g.pz == 1 && g.py == 1 && g.px == 1 && p.nzb == 1 && p.Zp == in.D + 2 && in.H == ge.geo - 2 && in.W == ge.geo - 2 &&
                                 a.vec_ok && Cin % 16 == 0) ? 1 : 0;
            }
    HIP_TRY(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsLimit));
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(c.WAVES * 64), p.lds_bytes, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) TH_FAIL(TH_EHIP, "conv_mfma launch failed: %s (%s)", hipGetErrorString(e), p.label.c_str());
    return TH_OK;
}
