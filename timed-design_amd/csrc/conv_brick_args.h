// Internal to conv_mfma.hip and conv_n16.hip: the argument struct of the two brick kernels, k_conv_mfma and k_conv_n16, and the LDS
// budget of their planners.  The kernels share no device code; they share the struct because both sit at the edge of the register
// file (most instantiations at 255-256 VGPRs, some spilling), where a changed kernarg offset changes the allocation.
//   k_conv_n16 only:  wx, in_grp_bytes
//   k_conv_mfma only: kd, kh, kw, ntaps, sd, sh, sw, n_mtiles, nnb, tab_off, zmajor, geo_compact, and dbg as a field (see its comment)
#pragma once
#include "common.h"

#include <cstring>

namespace {

constexpr size_t kLdsLimit = 160 * 1024;

struct ConvMfmaArgs {
    const float* in; int64_t in_fs; int in_cs, in_coff, Din, Hin, Win, Cin, vec_ok;
    int kd, kh, kw, pz, py, px, ntaps;
    int Dc, Hc, Wc;
    int FB, ZB, nzb, Zp, Hp, Wp, rows_pf, nrows, n_mtiles;
    int CS, nchunks, nnb, tab_off, zmajor;
    // TH_CONV_DBG timing knock-outs (the knock-out build only; results are WRONG when set): 1 only the first chunk is staged, 64 no
    // next-chunk prefetch in k_conv_n16.  k_conv_n16 reads it as TH_KNOCK (common.h).  k_conv_mfma reads the field itself, 0 in the
    // product build: with that one read folded to a constant seven of its TM = 4 instantiations, which spill already, spill one or
    // two VGPRs more (4 to 8 bytes of scratch per lane), so the field stays for it.
    int dbg;
    const float* wpk;
    int Cout;
    const float* bias;
    PreOp pre;
    PostOps post;
    float* out; int64_t out_fs; int out_cs, out_coff, Ho, Wo;
    int64_t nframes;
    const float* wx;   // k_conv_n16 XC > 0: weights of output channels 16..16+XC-1, [chunk][tap][q][c][4]
    int sd, sh, sw;    // convolution stride (k_conv_mfma only; 1 elsewhere)
    unsigned in_grp_bytes;   // k_conv_n16: bytes from a frame group's first input element to its last (buffer descriptor)
    int geo_compact;   // k_conv_mfma GEO kernels: chunks after the first re-stage real voxels only (see the staging loop)
};

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

// what both launchers fill alike: the views, the geometry, the same-named fields of either plan struct, weights and epilogue.  Each
// launcher then sets what only its kernel reads (the two lists above); a field the kernel never reads may hold anything, here zero.
template <class Plan>
ConvMfmaArgs brick_args(const Plan& p, int64_t n, const TView& in, const TView& out, const ConvGeom& g, int Cin, int Cout, const float* wpk,
                        const float* bias, const PreOp& pre, const PostOps& post) {
    ConvMfmaArgs a;
    std::memset(&a, 0, sizeof a);
    a.in = in.p; a.in_fs = in.fs; a.in_cs = in.cs; a.in_coff = in.coff;
    a.Din = in.D; a.Hin = in.H; a.Win = in.W; a.Cin = Cin;
    a.vec_ok = (in.cs % 4 == 0 && in.coff % 4 == 0 && in.fs % 4 == 0 && ((uintptr_t)in.p % 16) == 0) ? 1 : 0;
    a.kd = g.kd; a.kh = g.kh; a.kw = g.kw; a.pz = g.pz; a.py = g.py; a.px = g.px; a.ntaps = g.kd * g.kh * g.kw;
    a.sd = g.sd; a.sh = g.sh; a.sw = g.sw;
    a.Dc = p.Dc; a.Hc = p.Hc; a.Wc = p.Wc;
    a.FB = p.FB; a.ZB = p.ZB; a.nzb = p.nzb; a.Zp = p.Zp; a.Hp = p.Hp; a.Wp = p.Wp;
    a.rows_pf = p.rows_pf; a.nrows = p.FB * p.rows_pf; a.nchunks = p.nchunks;
    TH_KNOCK_SET(a, th_knobs_of(p.knobs).conv_dbg);
    a.wpk = wpk; a.Cout = Cout; a.bias = bias; a.pre = pre; a.post = post;
    a.out = out.p; a.out_fs = out.fs; a.out_cs = out.cs; a.out_coff = out.coff; a.Ho = out.H; a.Wo = out.W;
    a.nframes = n;
    return a;
}

}  // namespace
