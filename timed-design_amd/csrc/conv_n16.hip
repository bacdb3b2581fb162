// Narrow-output fused Conv3D for gfx950: Cout <= 16 (DenseNet/DenseCPD growth convolutions), 3x3x3, stride 1, with the same Keras
// block folded in as conv_mfma.hip's brick kernel (input prologue, bias, epilogue chain, 2x2x2 pool).  k_conv_n16 shares its
// argument struct with k_conv_mfma (conv_brick_args.h) and no device code.
// A 32-wide MFMA tile would spend half its columns on zero padding, so this kernel uses
// v_mfma_f32_16x16x4_f32 (same 64 FLOP/clk/SIMD rate): lane (i = l&15, q = l>>4) supplies
// A[i][k=q] / B[k=q][i]; with one ds_read_b128 it holds channels 4q..4q+3 of its voxel, i.e. the
// operands of 4 consecutive MFMAs (K order permuted identically in the packed weights).
// Weight fragments stream L2 -> registers through a 9-tap ring (slot refilled right after its last
// use, 9 taps = several microseconds ahead).  Workgroups are PERSISTENT: the row/voxel tables are
// built once, then the workgroup walks its frame groups; while the MFMAs of one 16-channel chunk run,
// the global loads of the next chunk (or of chunk 0 of the next frame group) are already in flight
// into registers and are written to LDS between two barriers, so staging latency never sits on the
// MFMA pipe even with a single workgroup per CU.  The tap loop is fully unrolled with A registers
// pinned by sched_barrier.
#include "conv_brick_args.h"
#include "device_math.h"

#include <algorithm>
#include <cstring>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4n __attribute__((ext_vector_type(4)));

// XC > 0: output channels 16..16+XC-1 (Cout = 17..20, e.g. the 20 amino-acid classes of a TIMED head) ride on
// v_mfma_f32_4x4x1_16B_f32 from the SAME A registers: the instruction is 16 independent 4x4 outer products (lane
// 4b+i supplies A_b[i] and B_b[i]; VGPR r of lane 4b+j receives D_b[r][j] — checked on hardware,
// tools/microbench/mfma_4x4x1_layout.hip).  With lane (i16, q) holding channels 4q..4q+3 of tile row i16, block
// b = 4q + (i16>>2) multiplies rows 4(i16>>2)..+3 at channel 4q+t by W[4q+t][16 + (i16&3)]: exactly 4 rows x 4 extra
// channels per block, nothing padded, 25 % more matrix-pipe time for 25 % more channels (a 32-wide tile would spend
// 12 of 32 columns on zeros; the round-1 version ran these channels as 64 scalar FMAs per tap per wave on the VALU
// pipe and could not afford the next-chunk prefetch).  The four blocks of a row group hold partial sums over the
// channel quarters q; they are added with two cross-lane exchanges in the epilogue.
// GEO > 0: Hp = Wp = GEO at compile time.  The 27 tap offsets then are immediates of the ds_read_b128 instructions
// instead of a scalar offset + one v_add_u32 per read: measured on the bare tap loop (tools/microbench/
// n16_tap_bench.hip) the address arithmetic alone costs 5-6 % of the matrix pipe (92 -> 98.6 % at TM = 8).
template <int WAVES, int TM, int POOL, int XC = 0, int GEO = 0>
__global__ void __launch_bounds__(WAVES * 64, WAVES == 4 ? 2 : 1) k_conv_n16(const ConvMfmaArgs a) {
    static_assert(XC == 0 || (XC == 4 && TM <= 4 && POOL == 0), "side channels: 4 channels (one 4x4x1 block column), ping-pong variant, no pooling");
    constexpr int NTHREADS = WAVES * 64;
    constexpr int CI = 16, CI4 = 4, NTAPS = 27;
    constexpr int BR = 9;                       // weight-ring depth (taps in flight)
    constexpr int PF = (TM <= 4) ? 6 : 8;     // float4 per thread of next-chunk prefetch (REAL voxels only, see pf_off)
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i16 = lane & 15, q = lane >> 4;
    constexpr int CS4 = 5;                    // kCS = 20 floats per staged voxel (launch_conv_n16 sets a.CS to it)

    const int vox_pf = a.Zp * a.Hp * a.Wp;   // staged (haloed) voxels per frame and z slab
    const int nvox = a.FB * vox_pf;
    float4* A4 = smem;
    // The three tables live INSIDE the staged image: a voxel occupies CS = 20 floats of which the fragment reads and the
    // staging writes touch 16; floats 16, 17, 18 of voxel i hold rowvox[i], rowout[i], voxsrc[i] (nrows <= nvox).  No
    // LDS beyond the image itself, so two slabs of a 10^3 frame (2 x 80 640 B) share a CU.
    int* tabs = reinterpret_cast<int*>(smem);
    const int TS = a.CS;
#define ROWVOX(i) tabs[(i) * TS + 16]
#define ROWOUT(i) tabs[(i) * TS + 17]
#define VOXSRC(i) tabs[(i) * TS + 18]

    // z slabs (nzb > 1): a unit of work is (frame group, slab); gridDim.x is a multiple of nzb, so a persistent
    // workgroup keeps its slab and the tables are still built once.  The planner only emits nzb = 1 today: two 4-wave
    // workgroups per CU on 5-plane slabs of a 10^3 frame (2 x 80 640 B) were measured at 124.0 TFLOP/s against 125.2
    // for one 8-wave workgroup on the whole frame — the extra halo planes eat what the overlap gives.
    const int zb = blockIdx.x % a.nzb;
    const int z0 = zb * a.ZB;
    const int ZBv = min(a.ZB, a.Dc - z0);

    // ---- tables, relative to the first frame of a group: built ONCE per (persistent) workgroup -------
    for (int v = tid; v < nvox; v += NTHREADS) {
        const int xl = v % a.Wp; int t = v / a.Wp;
        const int yl = t % a.Hp; t /= a.Hp;
        const int zl = t % a.Zp; const int f = t / a.Zp;
        const int zi = z0 + zl - a.pz, yi = yl - a.py, xi = xl - a.px;
        const bool ok = zi >= 0 && zi < a.Din && yi >= 0 && yi < a.Hin && xi >= 0 && xi < a.Win;
        VOXSRC(v) = ok ? f * (int)a.in_fs + ((zi * a.Hin + yi) * a.Win + xi) * a.in_cs : -1;
    }
    for (int r = tid; r < a.nrows; r += NTHREADS) {
        const int f = r / a.rows_pf, qq = r - f * a.rows_pf;
        int vox = 0, oo = -1;
        if (POOL == 0) {
            const int hw = a.Hc * a.Wc;
            if (qq < ZBv * hw) {
                const int zl = qq / hw, rem = qq - zl * hw, y = rem / a.Wc, x = rem - y * a.Wc;
                vox = ((f * a.Zp + zl) * a.Hp + y) * a.Wp + x;
                oo = f * (int)a.out_fs + (((z0 + zl) * a.Ho + y) * a.Wo + x) * a.out_cs;
            }
            ROWOUT(r) = oo;
        } else {
            const int pq = qq >> 3, mate = qq & 7;
            const int PH = a.Hc >> 1, PW = a.Wc >> 1;
            if (pq < (ZBv >> 1) * PH * PW) {
                const int pzz = pq / (PH * PW), rem = pq - pzz * (PH * PW), pyy = rem / PW, pxx = rem - pyy * PW;
                const int zl = 2 * pzz + (mate >> 2), y = 2 * pyy + ((mate >> 1) & 1), x = 2 * pxx + (mate & 1);
                vox = ((f * a.Zp + zl) * a.Hp + y) * a.Wp + x;
                oo = f * (int)a.out_fs + ((((z0 >> 1) + pzz) * a.Ho + pyy) * a.Wo + pxx) * a.out_cs;
            }
            if (mate == 0) ROWOUT(r >> 3) = oo;
        }
        ROWVOX(r) = vox;
    }
    __syncthreads();

    const int n_mt = a.nrows / 16;
    const int total_blocks = (n_mt + TM - 1) / TM;
    const int rounds = (total_blocks + WAVES - 1) / WAVES;
    const float4* wpk4 = reinterpret_cast<const float4*>(a.wpk) + lane;  // [chunk][tap][lane]
    const int co = i16;
    const bool cvalid = co < a.Cout;
    const int cc = cvalid ? co : 0;
    const float bv = a.bias ? a.bias[cc] : 0.f;
    const int nvec = nvox * CI4;
    const bool has_pre = a.pre.scale || a.pre.act != ACT_LINEAR;
    const int64_t ngroups = (a.nframes + a.FB - 1) / a.FB * a.nzb;   // units: (frame group, slab), slab fastest
    // next-chunk prefetch: when the whole staged image is <= PF float4 per thread, the global loads of the
    // NEXT chunk (or of chunk 0 of this workgroup's next frame group) are issued before the MFMA phase of the
    // current chunk and land in registers underneath it
    // Only voxels that exist in the input are prefetched: the halo of the staged image is written (with zeros) by
    // the first, plain staging pass of the workgroup and never changes afterwards, so re-writing it every chunk
    // (42 % of a 12^3 image, 64 % of a 7^3 one) would only cost load issue slots, registers and LDS writes.
    const int zlo = max(a.pz - z0, 0), ylo = max(a.py, 0), xlo = max(a.px, 0);
    const int nzr = min(a.Zp, a.Din + a.pz - z0) - zlo, nyr = min(a.Hp, a.Hin + a.py) - ylo, nxr = min(a.Wp, a.Win + a.px) - xlo;
    const int real_pf = nzr * nyr * nxr;          // real voxels of one staged frame
    const int nreal4 = a.FB * real_pf * CI4;
    const bool can_pf = rounds == 1 && nreal4 <= PF * NTHREADS && nzr > 0 && nyr > 0 && nxr > 0 && a.vec_ok && (a.Cin & 3) == 0 && !(TH_KNOCK(a) & 64);

    // nvalid: frames of the group that exist (the last group of a batch may be ragged)
    auto load_vec = [&](const float* inb, int nvalid, int ch, int i, bool* okp) -> float4 {
        float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
        int off = (i < nvec) ? VOXSRC(i / CI4) : -1;
        if (nvalid < a.FB && off >= 0 && (i / CI4) / vox_pf >= nvalid) off = -1;
        const int g = i % CI4;
        const int c0 = ch * CI + g * 4;
        *okp = off >= 0;
        if (off >= 0 && c0 < a.Cin) {
            const float* src = inb + ch * CI + off + g * 4;
            if (a.vec_ok && c0 + 4 <= a.Cin) {
                val = *reinterpret_cast<const float4*>(src);
            } else {
                val.x = src[0];
                if (c0 + 1 < a.Cin) val.y = src[1];
                if (c0 + 2 < a.Cin) val.z = src[2];
                if (c0 + 3 < a.Cin) val.w = src[3];
            }
        }
        return val;
    };
    auto store_vec = [&](int ch, int i, float4 val, bool ok) {
        if (i >= nvec) return;
        const int v = i / CI4, g = i % CI4;
        if (has_pre && ok) {
            const int c0 = ch * CI + g * 4;
            float e[4] = {val.x, val.y, val.z, val.w}, y[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = min(c0 + k, a.Cin - 1);
                y[k] = a.pre.scale ? fmaf(e[k], a.pre.scale[c], a.pre.shift[c]) : e[k];
            }
            th_act_vec<4>(y, a.pre.act, a.pre.alpha);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (c0 + k < a.Cin) e[k] = y[k];
            val = make_float4(e[0], e[1], e[2], e[3]);
        }
        A4[(size_t)v * CS4 + g] = val;
    };

    // weight ring: slot t % BR holds tap t's fragment and is refilled with tap t + BR right after its last
    // use.  The packed image is [chunk][tap][lane] + the first BR taps once more at the end, so the index simply runs
    // on (into the next chunk, and past the last chunk into the copy of chunk 0 for the next frame group) — and the
    // refill address is (uniform chunk base) + (one of 7 loop-invariant per-lane offsets) + (immediate): NO address
    // arithmetic in the tap loop.  On the bare loop 8 scalar + 1 vector instruction per refill cost 3-5 % of the
    // matrix pipe (tools/microbench/n16_tap_bench.hip).
    float4 breg[BR];
    unsigned voff[9];      // lane * 16 + k * 4096 bytes; (t + BR) * 1024 = voff[(t + BR) >> 2] + ((t + BR) & 3) * 1024
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        voff[k] = (unsigned)lane * 16u + (unsigned)k * 4096u;
        asm volatile("" : "+v"(voff[k]));   // keep them as registers: re-deriving them would put the adds back
    }
    // XC: this lane's B operand of the 4x4x1 blocks, xw[t % 3] = W_t[4q..4q+3][16 + (i16 & 3)] (packed image
    // [chunk][tap][q][c][4] + 3 taps of padding); a slot is refilled with tap t + 3 right after use (27 taps = 9 turns
    // of the ring, so slots line up across chunks)
    const f32x4* wx4 = reinterpret_cast<const f32x4*>(a.wx) + q * (XC ? XC : 1) + (XC ? (i16 & 3) : 0);
    unsigned voffx[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        voffx[k] = (unsigned)(q * (XC ? XC : 1) + (XC ? (i16 & 3) : 0)) * 16u + (unsigned)k * 4096u;
        asm volatile("" : "+v"(voffx[k]));
    }
    f32x4 xw[3];
    if (wave < total_blocks) {
#pragma unroll
        for (int t = 0; t < BR; ++t) breg[t] = wpk4[(size_t)t * 64];
        if (XC) {
#pragma unroll
            for (int r = 0; r < 3; ++r) xw[r] = wx4[(size_t)r * 4 * XC];
        }
    }

    // this thread's prefetch slots: BYTE offset (from the frame group's first input element) of the float4 it fetches for
    // real voxel (tid + u * NTHREADS) / 4, or OOB = nothing (the buffer load then returns zeros without touching memory)
    // — and where it goes in the staged image (float4 index).  The loads are buffer loads: a per-group descriptor, this
    // per-slot offset in a VGPR and the chunk's channel offset in an SGPR, i.e. NO address arithmetic and no select per
    // load in front of the MFMA phase (the 64-bit pointer form cost ~6 VALU instructions per load).
    constexpr unsigned OOB = 0xffffffffu;
    unsigned pf_boff[PF];
    int pf_dst[PF];
#pragma unroll
    for (int u = 0; u < PF; ++u) {
        const int i = tid + u * NTHREADS;
        pf_boff[u] = OOB; pf_dst[u] = 0;
        if (can_pf && i < nreal4) {
            const int r = i / CI4, f = r / real_pf, rr = r - f * real_pf;
            const int xa = rr % nxr, t = rr / nxr, ya = t % nyr, za = t / nyr;
            const int v = ((f * a.Zp + za + zlo) * a.Hp + ya + ylo) * a.Wp + xa + xlo;
            pf_boff[u] = (unsigned)(VOXSRC(v) + (i % CI4) * 4) * 4u;
            pf_dst[u] = v * CS4 + (i % CI4);
        }
    }
    bool staged = false;   // chunk 0 of the current group was already written to LDS from the prefetch registers
    for (int64_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const int64_t f0 = grp / a.nzb * a.FB;
        const int nvalid = (int)min((int64_t)a.FB, a.nframes - f0);
        const float* inb0 = a.in + f0 * a.in_fs + a.in_coff;
        float* outb = a.out + f0 * a.out_fs + a.out_coff;
        const int64_t gnext = grp + gridDim.x;   // same slab: gridDim.x % nzb == 0
        const bool has_next = gnext < ngroups;
        const int64_t f0_next = (has_next ? gnext : grp) / a.nzb * a.FB;
        const float* inb_next = a.in + f0_next * a.in_fs + a.in_coff;
        const int nvalid_next = has_next ? (int)min((int64_t)a.FB, a.nframes - f0_next) : nvalid;
        // a ragged group (the last one of a launch) takes the plain staging path, which knows about missing frames
        const bool grp_pf = can_pf && nvalid == a.FB && !(TH_KNOCK(a) & 1);
        const bool nxt_pf = can_pf && has_next && nvalid_next == a.FB && !(TH_KNOCK(a) & 1);
        const __amdgpu_buffer_rsrc_t rs_cur = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(inb0), 0, (int)a.in_grp_bytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t rs_nxt = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(inb_next), 0, (int)a.in_grp_bytes, 0x00020000);

        for (int rd = 0; rd < rounds; ++rd) {
            const int blk = rd * WAVES + wave;
            const bool active = blk < total_blocks;
            f32x4 acc[TM];
#pragma unroll
            for (int tm = 0; tm < TM; ++tm) acc[tm] = f32x4{0.f, 0.f, 0.f, 0.f};
            f32x4 xacc[XC ? TM : 1];   // 4x4x1 accumulators: VGPR r = row 4*(i16>>2)+r, this lane = extra channel i16&3, channel quarter q
#pragma unroll
            for (int tm = 0; tm < (XC ? TM : 1); ++tm) xacc[tm] = f32x4{0.f, 0.f, 0.f, 0.f};
            int aidx[TM];
#pragma unroll
            for (int tm = 0; tm < TM; ++tm) {
                const int mt = blk * TM + tm;
                aidx[tm] = ((active && mt < n_mt) ? ROWVOX(mt * 16 + i16) : 0) * CS4 + q;
            }
            for (int ch = 0; ch < a.nchunks; ++ch) {
                const bool need_a = !(a.nchunks == 1 && rd > 0) && !((TH_KNOCK(a) & 1) && (ch > 0 || grp != blockIdx.x));
                if (!(ch > 0 ? grp_pf : staged)) {   // otherwise this chunk was written from registers already
                    __syncthreads();
                    if (need_a) {
                        constexpr int U = 4;
                        for (int base = tid; base < nvec; base += NTHREADS * U) {
                            float4 val[U];
                            bool ok[U];
#pragma unroll
                            for (int u = 0; u < U; ++u) val[u] = load_vec(inb0, nvalid, ch, base + u * NTHREADS, &ok[u]);
#pragma unroll
                            for (int u = 0; u < U; ++u) store_vec(ch, base + u * NTHREADS, val[u], ok[u]);
                        }
                    }
                }
                __syncthreads();
                const bool last_ch = ch + 1 == a.nchunks;
                const bool do_pf = last_ch ? nxt_pf : grp_pf;
                const int pch = last_ch ? 0 : ch + 1;
                // The PF loads are issued UNCONDITIONALLY (also when their result will not be used): hipcc can then count
                // them and waits for the weight ring with vmcnt(N) instead of vmcnt(0), which would drain the prefetch in
                // front of the first MFMA.
                float4 pfv[PF];
                {
                    const int g = tid % CI4;                 // NTHREADS % CI4 == 0: the same channel group for every u
                    // nothing is fetched for channels past Cin in the last chunk, nor from a ragged group (frames that do not
                    // exist must not be touched; such a group is staged by the plain path)
                    const bool full = last_ch ? nvalid_next == a.FB : nvalid == a.FB;
                    const unsigned gmask = (full && pch * CI + g * 4 + 4 <= a.Cin) ? 0u : OOB;
                    const unsigned soff = (unsigned)(pch * CI) * 4u;
#pragma unroll
                    for (int u = 0; u < PF; ++u) {
                        const u32x4n raw = last_ch ? __builtin_amdgcn_raw_buffer_load_b128(rs_nxt, pf_boff[u] | gmask, soff, 0)
                                                   : __builtin_amdgcn_raw_buffer_load_b128(rs_cur, pf_boff[u] | gmask, soff, 0);
                        pfv[u] = __builtin_bit_cast(float4, raw);
                    }
                }
                // a thread's prefetched vectors all cover the same 4 channels (NTHREADS % 4 == 0): their BN constants
                // are fetched once, also unconditionally
                const int pc0 = min(pch * CI + (tid % CI4) * 4, a.Cin - 4);
                const bool pbn = a.pre.scale && can_pf;   // can_pf: Cin % 4 == 0, so pc0 is aligned and in bounds
                const float4 psc = *reinterpret_cast<const float4*>(pbn ? a.pre.scale + pc0 : a.wpk);
                const float4 psh = *reinterpret_cast<const float4*>(pbn ? a.pre.shift + pc0 : a.wpk);
                const char* wsc = reinterpret_cast<const char*>(a.wpk) + (size_t)ch * (NTAPS * 1024);          // uniform
                const char* wxs = reinterpret_cast<const char*>(a.wx) + (size_t)ch * (NTAPS * 4 * (XC ? XC : 1) * 16);
                if (active) {
                    // A fragments: TM <= 4 keeps two register sets (ping-pong by tap).  TM = 8 has ONE set and pipelines at
                    // half-tap granularity instead: as soon as the MFMAs of tiles 0..3 of tap t have issued, their
                    // registers are re-loaded with tap t+1 while the MFMAs of tiles 4..7 run (and vice versa), so every
                    // ds_read has 16 MFMAs (512 cycles) of cover without a second register set.
                    constexpr bool PING = (TM <= 4);
                    constexpr int HT = PING ? TM : TM / 2;
                    f32x4 av[PING ? 2 : 1][TM];
                    const f32x4* A4v = reinterpret_cast<const f32x4*>(A4);
#pragma unroll
                    for (int tm = 0; tm < TM; ++tm) av[0][tm] = A4v[aidx[tm]];
#pragma unroll
                    for (int t = 0; t < NTAPS; ++t) {
                        const int nt = t + 1;
                        int noff = (((nt / 9) * (GEO ? GEO : a.Hp) + (nt / 3) % 3) * (GEO ? GEO : a.Wp) + nt % 3) * CS4;
                        // runtime geometry: opaque to LICM, otherwise hipcc hoists all 27*TM read addresses out of the
                        // chunk loop and spills them to scratch
                        if (!GEO) asm volatile("" : "+s"(noff));
                        if (PING && nt < NTAPS) {
#pragma unroll
                            for (int tm = 0; tm < TM; ++tm) av[nt & 1][tm] = A4v[aidx[tm] + noff];
                        }
                        __builtin_amdgcn_sched_barrier(0);
                        if (!XC) {
#pragma unroll
                            for (int tm = 0; tm < HT; ++tm) {
                                const f32x4 aq = av[PING ? (t & 1) : 0][tm];
                                acc[tm] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq.x, breg[t % BR].x, acc[tm], 0, 0, 0);
                                acc[tm] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq.y, breg[t % BR].y, acc[tm], 0, 0, 0);
                                acc[tm] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq.z, breg[t % BR].z, acc[tm], 0, 0, 0);
                                acc[tm] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq.w, breg[t % BR].w, acc[tm], 0, 0, 0);
                            }
                        } else {
                            // k-major MFMA order (TM independent tiles between dependent accumulations); the 16-wide MFMA
                            // of (k, tm) is followed by the 4x4x1 MFMA of the same A register for the side channels
                            const float bk[4] = {breg[t % BR].x, breg[t % BR].y, breg[t % BR].z, breg[t % BR].w};
                            const f32x4 wv = xw[t % 3];
#pragma unroll
                            for (int k = 0; k < 4; ++k) {
#pragma unroll
                                for (int tm = 0; tm < TM; ++tm) {
                                    const f32x4 aq = av[t & 1][tm];
                                    acc[tm] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq[k], bk[k], acc[tm], 0, 0, 0);
                                    xacc[tm] = __builtin_amdgcn_mfma_f32_4x4x1f32(aq[k], wv[k], xacc[tm], 0, 0, 0);
                                }
                            }
                        }
                        __builtin_amdgcn_sched_barrier(0);
                        if (XC) {
                            const int xb = (t + 3) * 4 * XC * 16;   // bytes from the chunk's first tap
                            xw[t % 3] = *reinterpret_cast<const f32x4*>(wxs + voffx[xb >> 12] + (xb & 4095));
                        }
                        if (!PING) {
                            if (nt < NTAPS) {
#pragma unroll
                                for (int tm = 0; tm < HT; ++tm) av[0][tm] = A4v[aidx[tm] + noff];
                            }
                            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                            for (int tm = HT; tm < TM; ++tm) {
                                const f32x4 aq = av[0][tm];
                                acc[tm] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq.x, breg[t % BR].x, acc[tm], 0, 0, 0);
                                acc[tm] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq.y, breg[t % BR].y, acc[tm], 0, 0, 0);
                                acc[tm] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq.z, breg[t % BR].z, acc[tm], 0, 0, 0);
                                acc[tm] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq.w, breg[t % BR].w, acc[tm], 0, 0, 0);
                            }
                            __builtin_amdgcn_sched_barrier(0);
                        }
                        breg[t % BR] = *reinterpret_cast<const float4*>(wsc + voff[(t + BR) >> 2] + ((t + BR) & 3) * 1024);
                        if (!PING && nt < NTAPS) {
#pragma unroll
                            for (int tm = HT; tm < TM; ++tm) av[0][tm] = A4v[aidx[tm] + noff];
                        }
                    }
                }
                if (do_pf) {
                    // BN -> activation prologue in registers BEFORE the barrier (overlaps the other waves' last MFMAs).  The
                    // activation is decoded ONCE for all 4 PF values (th_act_vec): th_act's switch inlined per element
                    // cost ~10 scalar + vector instructions per value in this serial phase of the chunk.
                    if (has_pre && pch * CI + (tid % CI4) * 4 < a.Cin) {   // (a thread's vectors all cover the same 4 channels)
                        float xv[4 * PF];
#pragma unroll
                        for (int u = 0; u < PF; ++u) {
                            xv[4 * u] = pfv[u].x; xv[4 * u + 1] = pfv[u].y; xv[4 * u + 2] = pfv[u].z; xv[4 * u + 3] = pfv[u].w;
                        }
                        if (a.pre.scale) {
#pragma unroll
                            for (int u = 0; u < PF; ++u) {
                                xv[4 * u] = fmaf(xv[4 * u], psc.x, psh.x); xv[4 * u + 1] = fmaf(xv[4 * u + 1], psc.y, psh.y);
                                xv[4 * u + 2] = fmaf(xv[4 * u + 2], psc.z, psh.z); xv[4 * u + 3] = fmaf(xv[4 * u + 3], psc.w, psh.w);
                            }
                        }
                        th_act_vec<4 * PF>(xv, a.pre.act, a.pre.alpha);
#pragma unroll
                        for (int u = 0; u < PF; ++u) pfv[u] = make_float4(xv[4 * u], xv[4 * u + 1], xv[4 * u + 2], xv[4 * u + 3]);   // slots that fetched nothing are never stored
                    }
                    __syncthreads();   // every wave is done reading chunk ch
#pragma unroll
                    for (int u = 0; u < PF; ++u)
                        if (pf_boff[u] != OOB) A4[pf_dst[u]] = pfv[u];
                }
            }
            // ---- epilogue in registers: C layout col = lane&15, row = 4*(lane>>4) + reg --------------------
            if (active) {
#pragma unroll
                for (int g0 = 0; g0 < TM; g0 += 4) {
                    float x[16];
#pragma unroll
                    for (int g = 0; g < 4; ++g)
#pragma unroll
                        for (int r = 0; r < 4; ++r) x[4 * g + r] = (g0 + g < TM) ? acc[(g0 + g < TM) ? g0 + g : 0][r] + bv : 0.f;
                    th_post16(x, cc, a.post);
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        if (g0 + g >= TM) continue;
                        const int mt = blk * TM + g0 + g;
                        // rows of frames past the end of a ragged last group are dropped
                        const bool ok = cvalid && mt < n_mt && (nvalid == a.FB || (mt * 16 + 4 * q) / a.rows_pf < nvalid);
                        if (POOL == 0) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int oo = ok ? ROWOUT(mt * 16 + 4 * q + r) : -1;
                                if (oo >= 0) outb[oo + co] = x[4 * g + r];
                            }
                        } else {
                            // rows 4q..4q+3 of the tile = mates (4q)&7.. of pooled voxel q>>1: combine with lane q^1
                            float m;
                            if (POOL == 1) m = fmaxf(fmaxf(x[4 * g], x[4 * g + 1]), fmaxf(x[4 * g + 2], x[4 * g + 3]));
                            else m = (x[4 * g] + x[4 * g + 1]) + (x[4 * g + 2] + x[4 * g + 3]);
                            const float o2 = __shfl_xor(m, 16);
                            m = (POOL == 1) ? fmaxf(m, o2) : (m + o2) * 0.125f;
                            const int oo = ok ? ROWOUT(mt * 2 + (q >> 1)) : -1;
                            if (oo >= 0 && (q & 1) == 0) outb[oo + co] = m;
                        }
                    }
                }
                if (XC) {
                    // side channels: lane (q, g = i16>>2, j = i16&3) holds, in VGPR r, the partial sum of row 4g+r, channel
                    // 16+j over channel quarter q; add the four quarters (lanes 16 apart), then lane q finishes row 4g+q
                    const int cx = 16 + (i16 & 3);
                    const bool xvalid = cx < a.Cout;
                    const float bx = (a.bias && xvalid) ? a.bias[cx] : 0.f;
#pragma unroll
                    for (int tm = 0; tm < (XC ? TM : 1); ++tm) {
                        float mine = 0.f;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            float v = xacc[tm][r];
                            v += __shfl_xor(v, 16);
                            v += __shfl_xor(v, 32);
                            mine = (q == r) ? v : mine;
                        }
                        const int mt = blk * TM + tm;
                        const int row = mt * 16 + 4 * (i16 >> 2) + q;
                        const bool ok = xvalid && mt < n_mt && (nvalid == a.FB || row / a.rows_pf < nvalid);
                        const int oo = ok ? ROWOUT(row) : -1;
                        if (oo >= 0) outb[oo + cx] = th_post(mine + bx, cx, a.post);
                    }
                }
            }
        }
        staged = nxt_pf;
    }
}

#undef ROWVOX
#undef ROWOUT
#undef VOXSRC

// ---- planning, packing, launch ----------------------------------------------------------------------------------------------
typedef void (*ConvKernelN16)(const ConvMfmaArgs);
struct N16Cfg { int WAVES, TM; ConvKernelN16 k[3]; };   // k: the instantiation per pool mode
constexpr int kNumN16 = 3;
const N16Cfg kN16[kNumN16] = {
    {8, 8, {k_conv_n16<8, 8, 0>, k_conv_n16<8, 8, 1>, k_conv_n16<8, 8, 2>}},
    {4, 4, {k_conv_n16<4, 4, 0>, k_conv_n16<4, 4, 1>, k_conv_n16<4, 4, 2>}},
    {4, 4, {k_conv_n16<4, 4, 0, 4>, nullptr, nullptr}},   // with 4 side channels on 4x4x1 MFMA blocks (Cout 17..20), unpooled
};
// compile-time staged row geometry (Hp = Wp) for the shapes the DenseCPD / TIMED topologies use, unpooled
struct N16Geo { int variant, geo; ConvKernelN16 k; };
const N16Geo kN16Geo[] = {
    {0, 12, k_conv_n16<8, 8, 0, 0, 12>},
    {1, 7, k_conv_n16<4, 4, 0, 0, 7>},
    {2, 7, k_conv_n16<4, 4, 0, 4, 7>},
    {1, 4, k_conv_n16<4, 4, 0, 0, 4>},
};
constexpr int kCS = 20;   // floats per staged voxel: 16 channels + the three tables (see the kernel)

// the full instantiation, as rocprofv3 prints it: what the plan label and th_conv_brick_kernels name (variant 2: XC = 4)
std::string n16_kernel_name(int variant, int pool, int geo) {
    char buf[64];
    snprintf(buf, sizeof buf, "k_conv_n16<%d,%d,%d,%d,%d>", kN16[variant].WAVES, kN16[variant].TM, pool, variant == 2 ? 4 : 0, geo);
    return buf;
}

bool plan_n16(int variant, size_t lds_limit, const TView& in, const TView& oc, int Cin, int pool, const ThKnobs& kn, ConvN16Plan* p) {
    const N16Cfg& c = kN16[variant];
    p->knobs = &kn;
    p->variant = variant;
    p->nchunks = (Cin + 15) / 16; p->pool = pool;
    p->Dc = pool ? (oc.D / 2) * 2 : oc.D;
    p->Hc = pool ? (oc.H / 2) * 2 : oc.H;
    p->Wc = pool ? (oc.W / 2) * 2 : oc.W;
    p->Hp = p->Hc + 2; p->Wp = p->Wc + 2;
    auto rows_for = [&](int zb) { return round_up(pool ? 8 * ((zb / 2) * (p->Hc / 2) * (p->Wc / 2)) : zb * p->Hc * p->Wc, 16); };
    // the row / voxel tables live in the 4 spare floats of every staged voxel (CS = 20): the image is all the LDS there is
    auto lds_for = [&](int fb, int zb) { return (size_t)fb * (zb + 2) * p->Hp * p->Wp * kCS * 4; };
    const int max_mt = c.WAVES * c.TM;
    int FB = 1;
    const int ZB = p->Dc, nzb = 1;                                   // whole frames only (see the kernel on z slabs)
    if (lds_for(1, p->Dc) > lds_limit) return false;
    if (p->nchunks > 1 && rows_for(p->Dc) / 16 > max_mt) return false;
    while (FB < 32 && lds_for(FB + 1, p->Dc) <= lds_limit && (FB + 1) * rows_for(p->Dc) / 16 <= max_mt) ++FB;
    p->FB = FB; p->ZB = ZB; p->nzb = nzb; p->Zp = ZB + 2;
    p->rows_pf = rows_for(ZB);
    p->lds_bytes = lds_for(FB, ZB);
    if ((size_t)FB * p->rows_pf > (size_t)FB * p->Zp * p->Hp * p->Wp) return false;   // tables ride in the image: rows <= staged voxels
    const int xc = variant == 2 ? 4 : 0;   // side channels
    if (xc && pool) return false;
    p->xc = xc;
    // both images carry the first taps once more at the end (9 resp. 3: the ring depths), so the kernel's refill index never wraps
    p->wpk_floats = ((size_t)p->nchunks * 27 + 9) * 64 * 4 + (xc ? ((size_t)p->nchunks * 27 + 3) * 4 * xc * 4 : 0);
    p->exec_flops = 2.0 * (double)p->rows_pf * p->nzb * 16.0 * (double)(p->nchunks * 16) * 27;   // MFMA only
    if ((int64_t)FB * oc.fs > 0x7fffffffLL || (int64_t)FB * in.D * in.H * in.W * std::max(in.cs, in.C) > 0x7fffffffLL) return false;
    p->geo = 0;
    if (pool == 0 && p->Hp == p->Wp)
        for (const N16Geo& ge : kN16Geo)
            if (ge.variant == variant && ge.geo == p->Hp) p->geo = ge.geo;
    char buf[224];
    snprintf(buf, sizeof buf, "conv_n16<w%d,tm%d,pool%d%s> FB%d ZB%d/%d rows%d lds%zuK (16x16x4 MFMA, weight ring%s) [%s]",
             c.WAVES, c.TM, pool, xc ? ",xc4" : "", FB, ZB, p->Dc, p->rows_pf, p->lds_bytes / 1024,
             xc ? ", channels 16.. on 4x4x1 MFMA blocks" : "", n16_kernel_name(variant, pool, p->geo).c_str());
    p->label = buf;
    return true;
}

}  // namespace

// Cout <= 16: two 4-wave workgroups per CU when the frames fit in half the LDS, else one 8-wave workgroup; 17..20 unpooled: the XC form
bool conv_n16_plan(const TView& in, const TView& oc, const ConvGeom& g, int Cin, int Cout, int pool, const ThKnobs& kn, ConvN16Plan* p) {
    if (g.dd != 1 || g.dh != 1 || g.dw != 1 || g.sd != 1 || g.sh != 1 || g.sw != 1) return false;
    if (g.kd != 3 || g.kh != 3 || g.kw != 3 || Cin <= 8) return false;
    if (pool && (oc.D < 2 || oc.H < 2 || oc.W < 2)) return false;
    if (Cout <= 16) return plan_n16(1, kLdsLimit / 2, in, oc, Cin, pool, kn, p) || plan_n16(0, kLdsLimit, in, oc, Cin, pool, kn, p);
    if (Cout <= 20 && pool == 0) return plan_n16(2, kLdsLimit / 2, in, oc, Cin, pool, kn, p);
    return false;
}

// every compiled instantiation, one name per line: the non-null entries of kN16 x pool, then kN16Geo
void conv_n16_kernel_names(std::string* out) {
    for (int v = 0; v < kNumN16; ++v)
        for (int pool = 0; pool < 3; ++pool)
            if (kN16[v].k[pool]) *out += n16_kernel_name(v, pool, 0) + "\n";
    for (const N16Geo& ge : kN16Geo) *out += n16_kernel_name(ge.variant, 0, ge.geo) + "\n";
}

// Keras [3,3,3,Cin,Cout] -> [chunk][tap][q][j][t] with ci = chunk*16 + 4q + t, co = j
void conv_n16_pack_weights(const ConvN16Plan& p, int Cin, int Cout, const float* w, float* dst) {
    const int ntaps = 27;
    std::memset(dst, 0, p.wpk_floats * sizeof(float));
    for (int ch = 0; ch < p.nchunks; ++ch)
        for (int t = 0; t < ntaps; ++t)
            for (int q = 0; q < 4; ++q)
                for (int j = 0; j < 16 && j < Cout; ++j)
                    for (int e = 0; e < 4; ++e) {
                        const int ci = ch * 16 + 4 * q + e;
                        if (ci < Cin) dst[((((size_t)ch * ntaps + t) * 4 + q) * 16 + j) * 4 + e] = w[((size_t)t * Cin + ci) * Cout + j];
                    }
    std::memcpy(dst + (size_t)p.nchunks * ntaps * 256, dst, (size_t)9 * 256 * sizeof(float));   // ring run-on: taps 0..8 again
    // side channels: [chunk][tap][q][c][e] appended after the MFMA image
    const int xc = p.xc;
    float* wx = dst + ((size_t)p.nchunks * ntaps + 9) * 256;
    for (int ch = 0; ch < p.nchunks; ++ch)
        for (int t = 0; t < ntaps; ++t)
            for (int q = 0; q < 4; ++q)
                for (int c = 0; c < xc; ++c)
                    for (int e = 0; e < 4; ++e) {
                        const int ci = ch * 16 + 4 * q + e, co = 16 + c;
                        if (ci < Cin && co < Cout) wx[((((size_t)ch * ntaps + t) * 4 + q) * xc + c) * 4 + e] = w[((size_t)t * Cin + ci) * Cout + co];
                    }
    if (xc) std::memcpy(wx + (size_t)p.nchunks * ntaps * 4 * xc * 4, wx, (size_t)3 * 4 * xc * 4 * sizeof(float));
}

int launch_conv_n16(hipStream_t s, int64_t n, const ConvN16Plan& p, TView in, TView out, ConvGeom g, int Cin, int Cout,
                    const float* wpk, const float* bias, PreOp pre, PostOps post) {
    if (p.variant < 0 || p.variant >= kNumN16 || !kN16[p.variant].k[p.pool]) TH_FAIL(TH_EINVAL, "conv_n16: bad plan");
    const int waves = kN16[p.variant].WAVES;
    ConvMfmaArgs a = brick_args(p, n, in, out, g, Cin, Cout, wpk, bias, pre, post);
    a.CS = kCS; a.wx = wpk + ((size_t)p.nchunks * 27 + 9) * 256;
    a.in_grp_bytes = (unsigned)std::min<int64_t>(0xfffffff0LL, ((int64_t)(p.FB - 1) * in.fs + ((int64_t)in.D * in.H * in.W - 1) * in.cs + Cin) * 4);
    // persistent workgroups: one resident set, each walks groups blockIdx.x, +gridDim.x, ...
    int64_t resident = (int64_t)p.ncu * (waves == 4 ? 2 : 1);
    if (const int r = th_knobs_of(p.knobs).n16_resident) resident = std::max(1, r);   // tests: force multi-trip workgroups
    // units = (frame group, slab); equal trip counts: ceil(units / ceil(units / resident)) workgroups, and a
    // workgroup keeps its slab: the stride is a multiple of nzb
    const int64_t units = (n + p.FB - 1) / p.FB * p.nzb;
    const int64_t trips = (units + resident - 1) / resident;
    int64_t grid = std::max<int64_t>(1, (units + trips - 1) / std::max<int64_t>(trips, 1));
    grid = (grid + p.nzb - 1) / p.nzb * p.nzb;
    if (grid > 0x7fffffffLL) TH_FAIL(TH_EINVAL, "conv_n16: grid too large");
    ConvKernelN16 k = kN16[p.variant].k[p.pool];
    if (p.geo)
        for (const N16Geo& ge : kN16Geo)
            if (ge.variant == p.variant && ge.geo == p.geo) k = ge.k;
    HIP_TRY(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsLimit));
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(waves * 64), p.lds_bytes, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) TH_FAIL(TH_EHIP, "conv_n16 launch failed: %s (%s)", hipGetErrorString(e), p.label.c_str());
    return TH_OK;
}
