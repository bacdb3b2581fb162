// Pointwise (1x1x1, stride 1) fused Conv3D for gfx950 — the DenseCPD/DenseNet bottleneck and
// transition convolutions (BN -> ReLU -> Conv1^3 [-> AvgPool 2]; SURVEY.md §8(d) DenseCPD-synth,
// reference README.md:242-258 for the model family, predict.py:142 for the call that runs it).
//
// A 1x1x1 convolution is a plain GEMM  Y[M, Cout] = post(pre(X[M, Cin]) . W + b)  over M = frames x
// voxels rows with arithmetic intensity ~ Cin*Cout/(2(Cin+Cout)) FLOP/B ~ 18 for 80 -> 64: it sits at
// the ridge of the fp32-MFMA / HBM roofline, so it is built as a STREAMING kernel, not as the
// haloed-brick implicit GEMM of conv_mfma.hip:
//   * no LDS staging of activations and no barrier in the loop: lane (j = l&31, h = l>>5) reads the
//     4 channels its MFMA k-slot contracts straight from global memory (16 B per lane, all Cin/8
//     loads of a 32-row tile issued back to back so every 128 B line is fetched once);
//   * the whole weight matrix sits in LDS in MFMA fragment order (one conflict-free ds_read_b128 per
//     4 MFMAs), loaded once per workgroup; workgroups are persistent and stride over the row tiles;
//   * the BN->ReLU prologue is applied to the loaded registers, bias + {act | BN-affine}* to the
//     accumulators, and a 2x2x2 max/avg pool is reduced in registers: GEMM rows are grouped 8
//     pool-mates per output voxel, which the 32x32 accumulator layout puts in 4 registers of lane l
//     and 4 of lane l^32 -> one cross-half exchange;
//   * stores are 128 B per (row, 32-channel tile): lanes 0..31 hold consecutive channels of one row.
// v_mfma_f32_32x32x2_f32, exact fp32.  Four 4-wave workgroups per CU hide the load latency.
#include "common.h"
#include "device_math.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "conv_pointwise_k.h"

// k_conv_pw2 instantiations compiled in conv_pointwise_b.hip: chunk-blocked output (blk), "BN-affine -> ReLU" epilogue (epi = 2);
// never null, an entry without a kernel where the instantiation does not exist.  conv_pw2_extra_at: the i-th entry of its three
// tables, null past the end
const PwEntry* conv_pw2_extra(int blk, int epi, int kmi, int nti, int slot12);
const PwEntry* conv_pw2_extra_at(int i);

namespace {

// a dispatch-table entry carries the name of its instantiation: the step label and th_conv_pw_pick print what the table holds
#define PW1(K, N, P) {k_conv_pw<K, N, P>, K, 0, "k_conv_pw<" #K "," #N "," #P ">"}
#define PW1_ROW(K, N) {PW1(K, N, 0), PW1(K, N, 1), PW1(K, N, 2)}
#define PW2_ROW(K, N) {PW2_ENTRY(K, N, 0, 0, 0), PW2_ENTRY(K, N, 1, 0, 0), PW2_ENTRY(K, N, 2, 0, 0)}
// [kmax index: 4, 8, 16][nt index: 1, 2, 4][pool]
const PwEntry kPw[3][3][3] = {
    {PW1_ROW(4, 1), PW1_ROW(4, 2), PW1_ROW(4, 4)},
    {PW1_ROW(8, 1), PW1_ROW(8, 2), PW1_ROW(8, 4)},
    {PW1_ROW(16, 1), PW1_ROW(16, 2), PW1_ROW(16, 4)},
};
const PwEntry kPw2[3][3][3] = {
    {PW2_ROW(4, 1), PW2_ROW(4, 2), PW2_ROW(4, 4)},
    {PW2_ROW(8, 1), PW2_ROW(8, 2), PW2_ROW(8, 4)},
    {PW2_ROW(16, 1), PW2_ROW(16, 2), {PW_NONE, PW_NONE, PW_NONE}},   // 16 x 4: no room for the second register set
};
// 12 slots for 72..96 input channels (most of DenseCPD's bottleneck layers): two register sets of 12 float4 leave room for
// three workgroups per CU where 16 slots allow two
const PwEntry kPw2_12[2][3] = {PW2_ROW(12, 1), PW2_ROW(12, 2)};
const int kPwKmax[3] = {4, 8, 16};
const int kPwNt[3] = {1, 2, 4};
constexpr size_t kPwLdsLimit = 64 * 1024;

// THE dispatch rule: which instantiation runs a planned layer.  `in_cs`, `in_coff`, `in_fs` are the input view's voxel stride,
// channel offset and frame stride in floats; `relu_chain` says the epilogue is exactly "BN-affine -> ReLU"; `runtime_ok` stands for
// the two conditions only a launch can see, a 16-byte aligned input pointer and both views spanning less than 4 GiB.  Both
// always hold for arena tensors at test sizes (buffers come from hipMalloc, a chunk of activations is far below 4 GiB), so
// conv_pw_plan, conv_pw_label and th_conv_pw_pick pass true and the label names what launch_conv_pw runs.
const PwEntry& pw_pick(const ConvPwPlan& p, int Cin, int in_cs, int in_coff, int64_t in_fs, bool out_blk, bool relu_chain, bool runtime_ok) {
    const int kmi = p.kmi, nti = p.nti;
    const bool vec = in_cs % 4 == 0 && in_coff % 4 == 0 && in_fs % 4 == 0;
    // the pipelined buffer-addressing kernel when the views allow it (see k_conv_pw2), else k_conv_pw
    if (!(kPw2[kmi][nti][p.pool].k && vec && runtime_ok && Cin % 8 == 0 && p.K8 <= kPwKmax[kmi])) return kPw[kmi][nti][p.pool];
    const int slot12 = (p.K8 > 8 && p.K8 <= 12 && nti <= 1) ? 1 : 0;
    const PwEntry* e = slot12 ? &kPw2_12[nti][p.pool] : &kPw2[kmi][nti][p.pool];
    if (out_blk) e = conv_pw2_extra(1, 0, kmi, nti, slot12);
    if (p.pool == 0 && relu_chain) {
        const PwEntry* er = conv_pw2_extra(out_blk ? 1 : 0, 2, kmi, nti, slot12);
        if (er->k) e = er;
    }
    return *e;
}

bool pw_relu_chain(const PostOps& post) {
    return post.n == 2 && post.type[0] == POP_AFFINE && post.type[1] == POP_ACT && post.act[1] == ACT_RELU;
}

std::string pw_label(const ConvPwPlan& p, const PwEntry& e) {
    const bool pipe = std::strncmp(e.name, "k_conv_pw2", 10) == 0;
    char buf[224];
    snprintf(buf, sizeof buf, "conv_pw<k%d,nt%d,pool%d> K8=%d lds%zuK (streaming 1x1x1, weights in LDS%s) [%s]", e.kmax, kPwNt[p.nti],
             p.pool, p.K8, p.lds_bytes / 1024, pipe ? ", next tile prefetched, buffer addressing" : "", e.name);
    return buf;
}

// the input view as the pick rule reads it; the fusion pass plans before storage is assigned (cs = 0): a dense tensor of its own
void pw_view(const TView& in, int Cin, int* cs, int* coff, int64_t* fs) {
    *cs = in.cs > 0 ? in.cs : Cin;
    *coff = in.coff;
    *fs = in.cs > 0 ? in.fs : (int64_t)in.V() * Cin;
}

}  // namespace

bool conv_pw_plan(const TView& in, const TView& oc, const ConvGeom& g, int Cin, int Cout, int pool, const ThKnobs& kn, ConvPwPlan* p) {
    if (g.kd != 1 || g.kh != 1 || g.kw != 1) return false;
    if (g.sd != 1 || g.sh != 1 || g.sw != 1 || g.dd != 1 || g.dh != 1 || g.dw != 1) return false;
    if (pool && (oc.D < 2 || oc.H < 2 || oc.W < 2)) return false;
    if (Cout > 128 || Cin < 1) return false;
    const int nti = Cout <= 32 ? 0 : (Cout <= 64 ? 1 : 2);
    const int NT = kPwNt[nti];
    const int K8 = (Cin + 7) / 8;
    const int kmi = K8 <= 4 ? 0 : (K8 <= 8 ? 1 : 2);
    const size_t lds = (size_t)K8 * NT * 64 * 16 + (size_t)K8 * 8 * 2 * 4;
    if (lds > kPwLdsLimit) return false;
    p->knobs = &kn;
    p->kmi = kmi; p->nti = nti; p->K8 = K8; p->pool = pool;
    p->lds_bytes = lds;
    p->wpk_floats = (size_t)K8 * NT * 256;
    const int rows_pf = pool ? (oc.D / 2) * 2 * ((oc.H / 2) * 2) * ((oc.W / 2) * 2) : oc.D * oc.H * oc.W;   // even-trimmed when pooled
    p->exec_flops = 2.0 * (double)rows_pf * (double)(32 * NT) * (double)(K8 * 8);
    // the kernel of the view as it is known now, channels-last output, generic chain: conv_pw_label names the one that runs once
    // storage, blocking and the epilogue are decided
    int cs, coff; int64_t fs;
    pw_view(in, Cin, &cs, &coff, &fs);
    p->label = pw_label(*p, pw_pick(*p, Cin, cs, coff, fs, false, false, true));
    return true;
}

// Keras [1,1,1,Cin,Cout] -> fragment order [kk][ntile][h][j][q] with ci = kk*8 + 4h + q, co = ntile*32 + j
void conv_pw_pack_weights(const ConvPwPlan& p, int Cin, int Cout, const float* w, float* dst) {
    std::memset(dst, 0, p.wpk_floats * sizeof(float));
    const int K8 = p.K8, NT = kPwNt[p.nti];
    for (int kk = 0; kk < K8; ++kk)
        for (int nt = 0; nt < NT; ++nt) {
            float* frag = dst + ((size_t)kk * NT + nt) * 256;
            for (int h = 0; h < 2; ++h)
                for (int j = 0; j < 32; ++j) {
                    const int co = nt * 32 + j;
                    if (co >= Cout) continue;
                    for (int q = 0; q < 4; ++q) {
                        const int ci = kk * 8 + 4 * h + q;
                        if (ci < Cin) frag[(h * 32 + j) * 4 + q] = w[(size_t)ci * Cout + co];
                    }
                }
        }
}

// the plan's label for the instantiation that runs on this input view (misaligned channel slices take k_conv_pw), with
// chunk-blocked output or not, behind this epilogue chain
std::string conv_pw_label(const ConvPwPlan& p, const TView& in, int Cin, bool out_blk, const PostOps& post) {
    int cs, coff; int64_t fs;
    pw_view(in, Cin, &cs, &coff, &fs);
    return pw_label(p, pw_pick(p, Cin, cs, coff, fs, out_blk, pw_relu_chain(post), true));
}

int launch_conv_pw(hipStream_t s, int64_t n, const ConvPwPlan& p, TView in, TView out, int Cin, int Cout, const float* wpk,
                   const float* bias, PreOp pre, PostOps post) {
    const int kmi = p.kmi, nti = p.nti;
    if (kmi < 0 || kmi >= 3 || nti < 0 || nti >= 3) TH_FAIL(TH_EINVAL, "conv_pw: bad plan");
    if (n <= 0) return TH_OK;
    ConvPwArgs a;
    std::memset(&a, 0, sizeof a);
    a.in = in.p; a.in_fs = in.fs; a.in_cs = in.cs; a.in_coff = in.coff; a.Cin = Cin; a.K8 = p.K8;
    a.vec_ok = (in.cs % 4 == 0 && in.coff % 4 == 0 && in.fs % 4 == 0 && ((uintptr_t)in.p % 16) == 0) ? 1 : 0;
    a.V = in.D * in.H * in.W; a.H = in.H; a.W = in.W;
    a.in_dense = (in.fs == (int64_t)a.V * in.cs) ? 1 : 0;
    a.Vo = out.D * out.H * out.W; a.Ho = out.H; a.Wo = out.W;
    a.wpk = wpk; a.Cout = Cout; a.bias = bias; a.pre = pre; a.post = post;
    a.out = out.p; a.out_fs = out.fs; a.out_cs = out.cs; a.out_coff = out.coff;
    a.out_blk = out.blk;
    if (out.blk && (p.pool || out.blk != 4 || out.coff || out.cs != Cout || Cout % 4)) TH_FAIL(TH_EINVAL, "conv_pw: bad chunk-blocked output view");
    const int64_t out_v = p.pool ? a.Vo : a.V;
    a.out_dense = (out.fs == out_v * out.cs) ? 1 : 0;
    const int64_t nrows = p.pool ? n * a.Vo * 8 : n * a.V;
    if (nrows >= 0x7fffffffLL) TH_FAIL(TH_EINVAL, "conv_pw: %lld rows per launch exceed the 32-bit row index; lower the chunk size", (long long)nrows);
    a.nrows = (unsigned)nrows;
    a.ntiles = (unsigned)((nrows + 31) / 32);
    TH_KNOCK_SET(a, th_knobs_of(p.knobs).pw_dbg);
    const unsigned want = (a.ntiles + 3) / 4;
    unsigned grid = std::min(want, 256u * 8u);   // persistent: up to 8 workgroups per CU queued, waves stride over tiles
    if (const int r = th_knobs_of(p.knobs).pw_resident) grid = std::min(want, (unsigned)std::max(1, r));   // tests: force multi-trip waves
    const int64_t in_span = ((n - 1) * in.fs + (int64_t)(a.V - 1) * in.cs + in.coff + Cin) * 4;
    const int64_t out_span = ((n - 1) * out.fs + (out_v - 1) * out.cs + out.coff + Cout) * 4;
    const bool runtime_ok = ((uintptr_t)in.p % 16) == 0 && in_span < 0xfffffff0LL && out_span < 0xfffffff0LL;
    const PwEntry& e = pw_pick(p, Cin, in.cs, in.coff, in.fs, out.blk != 0, pw_relu_chain(post), runtime_ok);
    if (e.name[9] == '2') { a.in_bytes = (unsigned)in_span; a.out_bytes = (unsigned)out_span; }     // k_conv_pw2: buffer descriptors
    // the four per-wave transpose tiles only for the kernels that use them: k_conv_pw stores a blocked output element by element, and
    // with them its widest layers (96 -> 128: 49 920 bytes of weights) asked for 68 368 bytes, past the 64 KiB that conv_pw_plan checks
    hipLaunchKernelGGL(e.k, dim3(grid), dim3(256), p.lds_bytes + (e.blk ? 4 * 32 * 36 * 4 + 16 : 0), s, a);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) TH_FAIL(TH_EHIP, "conv_pw launch failed: %s (%s)", hipGetErrorString(err), e.name);
    return TH_OK;
}

// ---- the dispatch rule for tests (include/timed_hip.h) ----------------------------------------------------------------------
// the instantiation a Cin -> Cout pointwise layer runs on an input view of voxel stride in_cs (<= 0: Cin) at channel offset
// in_coff whose frame stride is a whole number of voxel rows; "" when conv_pw_plan refuses the layer
extern "C" int th_conv_pw_pick(int Cin, int Cout, int pool, int in_cs, int in_coff, int out_blk, int relu_chain, char* buf, size_t len) {
    if (!buf || !len || pool < 0 || pool > 2) TH_FAIL(TH_EINVAL, "th_conv_pw_pick: bad arguments");
    static const ThKnobs kn;
    const ConvGeom g{1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0};
    TView iv, ov;
    iv.D = iv.H = iv.W = ov.D = ov.H = ov.W = 2;
    iv.C = Cin; ov.C = Cout;
    iv.cs = in_cs > 0 ? in_cs : Cin; iv.coff = in_coff; iv.fs = (int64_t)iv.V() * iv.cs;
    ConvPwPlan p;
    buf[0] = 0;
    if (!conv_pw_plan(iv, ov, g, Cin, Cout, pool, kn, &p)) return TH_OK;
    snprintf(buf, len, "%s", pw_pick(p, Cin, iv.cs, iv.coff, iv.fs, out_blk != 0, relu_chain != 0, true).name);
    return TH_OK;
}

// every compiled instantiation, one name per line: the non-null entries of the dispatch tables of this file and of conv_pointwise_b.hip
extern "C" int th_conv_pw_kernels(char* buf, size_t len) {
    if (!buf || !len) TH_FAIL(TH_EINVAL, "th_conv_pw_kernels: bad arguments");
    std::string all;
    auto add = [&](const PwEntry& e) { if (e.k) { all += e.name; all += "\n"; } };
    for (int kmi = 0; kmi < 3; ++kmi)
        for (int nti = 0; nti < 3; ++nti)
            for (int pool = 0; pool < 3; ++pool) { add(kPw[kmi][nti][pool]); add(kPw2[kmi][nti][pool]); }
    for (int nti = 0; nti < 2; ++nti)
        for (int pool = 0; pool < 3; ++pool) add(kPw2_12[nti][pool]);
    for (int i = 0; const PwEntry* e = conv_pw2_extra_at(i); ++i) add(*e);
    if (all.size() + 1 > len) TH_FAIL(TH_EINVAL, "th_conv_pw_kernels: %zu bytes needed", all.size() + 1);
    std::memcpy(buf, all.c_str(), all.size() + 1);
    return TH_OK;
}
