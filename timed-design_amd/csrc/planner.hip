// Pack parser and layer-graph planner (fusion + zero-copy concat): th_model's nodes -> its steps.
// The reference hands the network to TensorFlow as an opaque graph; here the graph is planned once
// at load time into a short list of launches:
//   * Conv3D + bias + {ELU/ReLU, BatchNorm}* + MaxPool/AvgPool(2) -> ONE fused MFMA kernel
//     (conv_mfma.hip); a BN->ReLU in FRONT of a conv (DenseNet/DenseCPD pre-activation) becomes the
//     kernel's staging prologue;
//   * Concatenate is zero-copy: producers write straight into a channel slice of the concat
//     buffer (nested concats collapse into one buffer per dense block);
//   * everything else runs on the generic kernels (kernels_generic.hip).
// Activations live in HBM as channels-last fp32, one arena per tensor sized for `chunk` frames.
#include "model.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <set>

using namespace th_rt;

namespace {
struct PackNode {
    uint32_t op, n_in;
    int32_t in[kMaxIn];
    int32_t ip[kNIp];
    float fp[kNFp];
    int32_t w[kNW];
    char name[kNameBytes];
};
static_assert(sizeof(PackNode) == 256, "pack node record must be 256 bytes");
struct PackHeader {
    char magic[8];
    uint32_t n_nodes, n_blobs, output_node, reserved;
};

inline void keras_same_pad(int n, int k, int s, int d, int* before) {
    const int ke = (k - 1) * d + 1;
    const int out = (n + s - 1) / s;
    int total = (out - 1) * s + ke - n;
    if (total < 0) total = 0;
    *before = total / 2;
}
}  // namespace

int th_rt::upload(th_model* m, const float* h, size_t count, float** out) {
    float* d = nullptr;
    if (int rc = cached_malloc((void**)&d, (count ? count : 1) * sizeof(float), m->device)) return rc;
    m->dev_allocs.push_back(d);
    if (count) HIP_TRY(hipMemcpy(d, h, count * sizeof(float), hipMemcpyHostToDevice));
    *out = d;
    return TH_OK;
}

int th_rt::parse_pack(th_model* m) {
    const std::vector<char>& p = m->pack;
    if (p.size() < sizeof(PackHeader)) TH_FAIL(TH_EIO, "pack too small (%zu bytes)", p.size());
    PackHeader h;
    std::memcpy(&h, p.data(), sizeof h);
    if (std::memcmp(h.magic, "THPK0001", 8) != 0) TH_FAIL(TH_EIO, "bad pack magic");
    size_t pos = sizeof(PackHeader);
    if (p.size() < pos + (size_t)h.n_nodes * sizeof(PackNode) + (size_t)h.n_blobs * 16) TH_FAIL(TH_EIO, "truncated pack");
    m->nodes.resize(h.n_nodes);
    for (uint32_t i = 0; i < h.n_nodes; ++i) {
        PackNode pn;
        std::memcpy(&pn, p.data() + pos, sizeof pn);
        pos += sizeof pn;
        Node& n = m->nodes[i];
        n.op = (int)pn.op;
        if (pn.n_in > (uint32_t)kMaxIn) TH_FAIL(TH_EIO, "node %u: too many inputs", i);
        for (uint32_t k = 0; k < pn.n_in; ++k) {
            if (pn.in[k] < 0 || pn.in[k] >= (int)i) TH_FAIL(TH_EIO, "node %u: input %d is not topologically earlier", i, pn.in[k]);
            n.in.push_back(pn.in[k]);
        }
        std::memcpy(n.ip, pn.ip, sizeof n.ip);
        std::memcpy(n.fp, pn.fp, sizeof n.fp);
        std::memcpy(n.w, pn.w, sizeof n.w);
        pn.name[kNameBytes - 1] = 0;
        n.name = pn.name;
        n.rank = pn.ip[kNIp - 5];
        const int* shp = &pn.ip[kNIp - 4];
        if (n.rank == 4) { n.D = shp[0]; n.H = shp[1]; n.W = shp[2]; n.C = shp[3]; }
        else if (n.rank == 1) { n.D = n.H = n.W = 1; n.C = shp[0]; }
        else TH_FAIL(TH_EUNSUP, "node %s: output rank %d not supported", n.name.c_str(), n.rank);
        if (n.C <= 0 || n.D <= 0 || n.H <= 0 || n.W <= 0) TH_FAIL(TH_EIO, "node %s: bad shape", n.name.c_str());
    }
    std::vector<std::pair<uint64_t, uint64_t>> table(h.n_blobs);
    for (uint32_t i = 0; i < h.n_blobs; ++i) {
        std::memcpy(&table[i].first, p.data() + pos, 8);
        std::memcpy(&table[i].second, p.data() + pos + 8, 8);
        pos += 16;
    }
    pos = (pos + 15) / 16 * 16;
    const size_t data_floats = (p.size() - pos) / 4;
    for (auto& t : table) {
        if (t.first + t.second > data_floats) TH_FAIL(TH_EIO, "blob outside pack data");
        m->blob_host.push_back(reinterpret_cast<const float*>(p.data() + pos) + t.first);
        m->blob_count.push_back((size_t)t.second);
    }
    if (h.output_node >= h.n_nodes) TH_FAIL(TH_EIO, "bad output node");
    m->output_node = (int)h.output_node;
    for (size_t i = 0; i < m->nodes.size(); ++i) {
        for (int s : m->nodes[i].in) m->nodes[s].consumers.push_back((int)i);
        for (int k = 0; k < kNW; ++k)
            if (m->nodes[i].w[k] >= (int)m->blob_host.size()) TH_FAIL(TH_EIO, "node %zu: blob index out of range", i);
        if (m->nodes[i].op == OP_INPUT) {
            if (m->input_node >= 0) TH_FAIL(TH_EUNSUP, "more than one model input");
            m->input_node = (int)i;
        }
    }
    if (m->input_node < 0) TH_FAIL(TH_EIO, "no input node");
    const Node& in = m->nodes[m->input_node];
    if (in.rank != 4) TH_FAIL(TH_EUNSUP, "input must be rank 4 (D,H,W,C)");
    m->in_dims[0] = in.D; m->in_dims[1] = in.H; m->in_dims[2] = in.W; m->in_dims[3] = in.C;
    const Node& on = m->nodes[m->output_node];
    if (on.rank != 1) TH_FAIL(TH_EUNSUP, "model output must be a vector per frame (got rank %d)", on.rank);
    m->n_classes = on.C;
    return TH_OK;
}

namespace {

bool is_elementwise(const Node& n) {
    return (n.op == OP_ACT && n.ip[0] != ACT_SOFTMAX) || n.op == OP_BN;
}

// fold BatchNormalization into scale/shift device vectors
int bn_affine(th_model* m, const Node& bn, const float** scale, const float** shift) {
    const int C = bn.ip[0];
    const float eps = bn.fp[0];
    auto blob = [&](int k) -> const float* { return bn.w[k] >= 0 ? m->blob_host[bn.w[k]] : nullptr; };
    const float *g = blob(0), *b = blob(1), *mu = blob(2), *var = blob(3);
    if (!mu || !var) TH_FAIL(TH_EIO, "%s: missing moving statistics", bn.name.c_str());
    for (int k = 0; k < 4; ++k)
        if (bn.w[k] >= 0 && (int)m->blob_count[bn.w[k]] != C) TH_FAIL(TH_EIO, "%s: BN vector length", bn.name.c_str());
    std::vector<float> sc(C), sh(C);
    for (int c = 0; c < C; ++c) {
        const float inv = (g ? g[c] : 1.f) / std::sqrt(var[c] + eps);
        sc[c] = inv;
        sh[c] = (b ? b[c] : 0.f) - mu[c] * inv;
    }
    float *dsc, *dsh;
    int rc;
    if ((rc = upload(m, sc.data(), C, &dsc)) || (rc = upload(m, sh.data(), C, &dsh))) return rc;
    *scale = dsc;
    *shift = dsh;
    return TH_OK;
}

// the activation `act` (slope `alpha`) at the end of an epilogue chain that has room for it
void add_act(PostOps* po, int act, float alpha) {
    const int i = po->n++;
    if (i == 0) po->monotone = 1;
    po->type[i] = POP_ACT;
    po->act[i] = act;
    po->alpha[i] = alpha;
    const bool mono = act == ACT_LINEAR || act == ACT_RELU || act == ACT_SIGMOID || act == ACT_TANH ||
                      ((act == ACT_ELU || act == ACT_LEAKY) && alpha >= 0.f);
    if (!mono) po->monotone = 0;
}

int add_post(th_model* m, PostOps* po, const Node& n) {
    if (po->n >= TH_MAX_POST) return 1;
    if (n.op != OP_BN) { add_act(po, n.ip[0], n.fp[0]); return TH_OK; }
    const int i = po->n;
    if (i == 0) po->monotone = 1;
    po->type[i] = POP_AFFINE;
    if (int rc = bn_affine(m, n, &po->scale[i], &po->shift[i])) return rc;
    // scale = gamma * rsqrt(var + eps): its sign is gamma's
    const float* g = n.w[0] >= 0 ? m->blob_host[n.w[0]] : nullptr;
    for (int c = 0; g && c < n.ip[0]; ++c) if (!(g[c] >= 0.f)) po->monotone = 0;
    po->n++;
    return TH_OK;
}

// the epilogue of output channels [c0, ...): its per-channel scale / shift vectors start at channel c0
PostOps post_from(PostOps po, int c0) {
    for (int k = 0; k < po.n; ++k) {
        if (po.scale[k]) po.scale[k] += c0;
        if (po.shift[k]) po.shift[k] += c0;
    }
    return po;
}

// a weight image of `floats` floats (zeroed), filled on the host by `pack`, then uploaded
template <class Pack>
int upload_packed(th_model* m, size_t floats, Pack pack, float** out) {
    std::vector<float> h(floats);
    pack(h.data());
    return upload(m, h.data(), h.size(), out);
}

// output channels [c0, c0 + cn) of Keras weights with `ktaps` rows of Cout
std::vector<float> weight_columns(const float* w, size_t ktaps, int Cout, int c0, int cn) {
    std::vector<float> out(ktaps * cn);
    for (size_t r = 0; r < ktaps; ++r) std::memcpy(&out[r * cn], w + r * Cout + c0, (size_t)cn * sizeof(float));
    return out;
}

// node n's shape as a dense channels-last view without storage: what the kernel planners size their tiles by
TView shape_of(const Node& n) {
    TView v;
    v.D = n.D; v.H = n.H; v.W = n.W; v.C = n.C;
    v.fs = (int64_t)n.D * n.H * n.W * n.C;
    return v;
}

ConvGeom conv_geom(const Node& c, const Node& in) {
    ConvGeom g{};
    g.kd = c.ip[0]; g.kh = c.ip[1]; g.kw = c.ip[2]; g.sd = c.ip[3]; g.sh = c.ip[4]; g.sw = c.ip[5];
    g.dd = c.ip[6]; g.dh = c.ip[7]; g.dw = c.ip[8];
    g.pz = g.py = g.px = 0;
    if (c.ip[9]) {
        keras_same_pad(in.D, g.kd, g.sd, g.dd, &g.pz);
        keras_same_pad(in.H, g.kh, g.sh, g.dh, &g.py);
        keras_same_pad(in.W, g.kw, g.sw, g.dw, &g.px);
    }
    return g;
}

struct ConvFusion {
    int src = -1;            // node whose output the conv reads (after absorbing a BN/act prologue)
    std::vector<int> pre;    // prologue nodes absorbed (in graph order)
    std::vector<int> post;   // epilogue nodes absorbed (in graph order)
    int pool = -1;           // pool node absorbed
    int last = -1;           // node whose tensor the step produces
};

// the kernel family that runs a Conv3D / Dense layer
enum class Kern { None, Wino, WfSplit, Wf, First5, First, Pointwise, Gl, N16, Mfma, Direct, DenseGemm, Dense };

// one Conv3D / Dense step: what it absorbs, and the kernel that runs it — decided once, read by every pass after the decision
struct LayerPlan {
    ConvFusion f;
    ConvGeom g{};                 // Conv3D: the geometry on the input it reads (f.src)
    Kern family = Kern::None;     // fusion pass: First5 / First / Pointwise / N16 / Mfma, each with its own plan (None: no MFMA-family plan)
    ConvFirstPlan fp;             // First
    ConvPwPlan pw;                // Pointwise
    ConvN16Plan np;               // N16
    ConvMfmaPlan mp;              // Mfma
    bool wf = false;              // conv_wfused serves the layer, with `wfp`
    ConvWfPlan wfp;
    Kern kind = Kern::None;       // what runs it (choose_kernel)
    ConvWinoPlan wp;              // Wino
    ConvWfsPlan sp;               // WfSplit
    bool b3 = false;              // First: on the bf16 pipe with split operands (conv_first_b3.hip)
    bool tailed = false;          // Mfma: the last Cout block, from channel `cout_main` on, runs on the narrower `tp`
    ConvMfmaPlan tp;
    int cout_main = 0;
    PostOps po;                   // the layer's own activation + the absorbed elementwise chain
    PreOp pre;                    // the absorbed BN -> activation in front of a convolution
    bool split_softmax = false;   // activation='softmax': a softmax step of its own after the layer
};

// the minimal-filtering and split-operand forms: what the load-time guard checks against a direct plan
bool fast_form(const LayerPlan& L) {
    return L.kind == Kern::Wino || L.kind == Kern::Wf || L.kind == Kern::WfSplit || L.kind == Kern::First5 ||
           (L.kind == Kern::First && (L.fp.first_wino || L.b3));
}

struct Planner {
    th_model* m;
    std::vector<Node>& N;
    const ThKnobs& kn;
    const bool fuse, use_mfma;
    std::map<int, LayerPlan> layers;   // by Conv3D / Dense node
    std::vector<char> concat_copy;     // [i * kMaxIn + k]: input k of concat i needs an explicit copy
    int fused_tail = -1;               // the final Softmax node when it was folded into the GlobalAveragePooling3D step
    std::set<int> wino_in_done;        // Winograd convolutions whose input transform was fused into the previous layer's output transform
    std::set<int> gap_done;            // GlobalAveragePooling3D nodes already computed by the output transform of the Winograd layer in front
    std::set<int> tail_done;           // nodes computed by a k_tail_dense step ([BN / act]* -> GAP -> Dense -> Softmax in one launch)
    explicit Planner(th_model* model)
        : m(model), N(model->nodes), kn(model->knobs), fuse(!(model->flags & (TH_LOAD_NO_FUSE | TH_LOAD_KEEP_ALL))),
          use_mfma(!(model->flags & TH_LOAD_NO_MFMA)), concat_copy(model->nodes.size() * kMaxIn, 0) {}
    int pool_mode(const ConvFusion& f) const { return f.pool < 0 ? 0 : N[f.pool].op == OP_MAXPOOL ? 1 : 2; }   // 0 none, 1 max, 2 avg
    void add_step(Step s) { m->steps.push_back(std::move(s)); }
    int new_buffer(int64_t floats_per_frame) {
        m->bufs.push_back(Buffer());
        m->bufs.back().floats_per_frame = floats_per_frame;
        return (int)m->bufs.size() - 1;
    }
    Step& add_step(int out_node, std::string label, double bytes, std::function<int(hipStream_t, int64_t)> run) {
        Step s;
        s.out_node = out_node; s.label = std::move(label); s.bytes = bytes; s.run = std::move(run);
        m->steps.push_back(std::move(s));
        return m->steps.back();
    }
};

// ---------------- pass 1: fusion decisions (symbolic) ----------------------------------------------------------------------
ConvFusion fuse_chain(const Planner& P, int i) {
    const std::vector<Node>& N = P.N;
    const Node& n = N[i];
    ConvFusion f;
    f.src = n.in[0];
    f.last = i;
    if (!P.fuse) return f;
    if (n.op == OP_CONV3D) {
        // prologue: [BN] -> [act] directly in front, each consumed only by this chain
        int x = f.src;
        std::vector<int> pre;
        if (N[x].absorbed_by < 0 && N[x].op == OP_ACT && N[x].ip[0] != ACT_SOFTMAX && N[x].consumers.size() == 1) {
            pre.push_back(x);
            x = N[x].in[0];
        }
        if (N[x].absorbed_by < 0 && N[x].op == OP_BN && N[x].consumers.size() == 1 && (pre.empty() || N[pre.back()].in[0] == x)) {
            pre.push_back(x);
            x = N[x].in[0];
        }
        if (!pre.empty()) {
            std::reverse(pre.begin(), pre.end());
            f.pre = pre;
            f.src = x;
        }
    }
    // activation='softmax' runs as a step of its own after the layer (LayerPlan::split_softmax), in place on the layer's output:
    // whatever follows it must read the probabilities, so no epilogue chain and no pool join the layer
    if ((n.op == OP_CONV3D ? n.ip[13] : n.ip[3]) == ACT_SOFTMAX) return f;
    // epilogue: elementwise chain with single consumers
    int cur = i;
    int npost = (n.op == OP_CONV3D ? n.ip[13] : n.ip[3]) != ACT_LINEAR ? 1 : 0;
    while (N[cur].consumers.size() == 1 && cur != P.m->output_node) {
        const int nx = N[cur].consumers[0];
        if (!is_elementwise(N[nx]) || npost >= TH_MAX_POST) break;
        f.post.push_back(nx);
        ++npost;
        cur = nx;
    }
    f.last = cur;
    if (n.op == OP_CONV3D && N[cur].consumers.size() == 1 && cur != P.m->output_node) {
        const Node& pl = N[N[cur].consumers[0]];
        if ((pl.op == OP_MAXPOOL || pl.op == OP_AVGPOOL) && pl.ip[0] == 2 && pl.ip[1] == 2 && pl.ip[2] == 2 &&
            pl.ip[3] == 2 && pl.ip[4] == 2 && pl.ip[5] == 2 && pl.ip[6] == 0)
            f.pool = N[cur].consumers[0];
    }
    return f;
}

// the MFMA family of convolution i, in this order: first5 -> first -> pointwise -> n16 -> mfma.  The brick kernels (n16, mfma) are
// tried with the fused pool first and then without it; the pool is dropped when the kernel that takes the layer cannot pool it.
void choose_family(const Planner& P, int i, LayerPlan& L) {
    ConvFusion& f = L.f;
    const Node& n = P.N[i];
    const Node& src = P.N[f.src];
    const ConvGeom& g = L.g;
    const TView iv = shape_of(src), ov = shape_of(n);
    const int pool = P.pool_mode(f);
    const bool stem = P.use_mfma && P.fuse && f.src == P.m->input_node && f.pre.empty();
    Kern& k = L.family;
    // ProDCoNN's 5x5x5 stem: direct form on the bf16 pipe, input split once at staging (conv_first5.hip)
    if (stem && pool == 1 && conv_first5_ok(src.D, src.H, src.W, src.C, n.C, g, 1, P.kn)) k = Kern::First5;
    if (k == Kern::None && stem && conv_first_plan(src.D, src.H, src.W, src.C, ov, g, n.C, pool, P.kn, &L.fp)) k = Kern::First;
    if (k == Kern::None && P.use_mfma && g.kd * g.kh * g.kw == 1 && conv_pw_plan(iv, ov, g, src.C, n.C, pool, P.kn, &L.pw))
        k = Kern::Pointwise;
    auto brick = [&](int pl) {    // one pool value (conv_brick_plan, which th_conv_brick_pick exports)
        const int b = conv_brick_plan(iv, ov, g, src.C, n.C, pl, P.kn, &L.np, &L.mp);
        return b == 1 ? Kern::N16 : b == 2 ? Kern::Mfma : Kern::None;
    };
    if (k == Kern::None && P.use_mfma) {
        if (f.pool >= 0) k = brick(pool);
        if (k == Kern::None && (k = brick(0)) != Kern::None) f.pool = -1;
    }
    if (k == Kern::None) f.pool = -1;
}

void fusion_pass(Planner& P) {
    std::vector<Node>& N = P.N;
    th_model* m = P.m;
    for (int i = 0; i < (int)N.size(); ++i) {
        Node& n = N[i];
        if (n.absorbed_by >= 0 || (n.op != OP_CONV3D && n.op != OP_DENSE)) continue;
        LayerPlan& L = P.layers[i];
        L.f = fuse_chain(P, i);
        if (n.op == OP_CONV3D) {
            L.g = conv_geom(n, N[L.f.src]);
            choose_family(P, i, L);
        }
        ConvFusion& f = L.f;
        if (f.pool >= 0) f.last = f.pool;
        for (int x : f.pre) N[x].absorbed_by = i;
        for (int x : f.post) N[x].absorbed_by = i;
        if (f.pool >= 0) N[f.pool].absorbed_by = i;
        if (f.last != i) n.absorbed_by = i;  // the conv's own raw output is never materialised
    }
    // does anything still need the converted fp32 copy of the input?  (the first-layer kernels read the caller's frames)
    m->need_convert = m->output_node == m->input_node;
    for (int c : N[m->input_node].consumers) {
        const auto it = P.layers.find(c);
        if (it == P.layers.end() || it->second.f.src != m->input_node ||
            (it->second.family != Kern::First && it->second.family != Kern::First5))
            m->need_convert = true;
    }
    // which node outputs exist in memory
    for (Node& n : N) n.materialised = n.absorbed_by < 0;
    for (auto& kv : P.layers) N[kv.second.f.last].materialised = true;
}

// ---------------- pass 2: storage (zero-copy concat, flatten aliasing) -------------------------------------------------------
void storage_pass(Planner& P) {
    std::vector<Node>& N = P.N;
    const int nn = (int)N.size();
    for (int i = nn - 1; i >= 0; --i) {
        Node& n = N[i];
        if (n.op != OP_CONCAT) continue;
        if (n.buf < 0) {
            n.cs = n.C; n.coff = 0;
            n.buf = P.new_buffer((int64_t)n.D * n.H * n.W * n.cs);
        }
        int off = 0;
        for (size_t k = 0; k < n.in.size(); ++k) {
            Node& a = N[n.in[k]];
            const bool can_alias = P.fuse && a.buf < 0 && a.materialised && a.op != OP_INPUT && a.op != OP_FLATTEN &&
                                   a.op != OP_IDENTITY;
            if (can_alias) {
                a.buf = n.buf; a.cs = n.cs; a.coff = n.coff + off;
            } else {
                P.concat_copy[i * kMaxIn + k] = 1;
            }
            off += a.C;
        }
    }
    for (int i = 0; i < nn; ++i) {
        Node& n = N[i];
        if (!n.materialised || n.buf >= 0) continue;
        if ((n.op == OP_FLATTEN || n.op == OP_IDENTITY)) {
            const Node& a = N[n.in[0]];
            if (a.cs == a.C && a.coff == 0) {  // contiguous: pure reinterpretation
                n.buf = a.buf; n.cs = n.C; n.coff = 0;
                if (n.op == OP_IDENTITY) { n.cs = a.cs; }
                continue;
            }
        }
        n.cs = n.C; n.coff = 0;
        if (n.op == OP_INPUT) {
            bool all_conv = !n.consumers.empty();
            for (int c : n.consumers) if (N[c].op != OP_CONV3D) all_conv = false;
            if (all_conv && P.fuse) n.cs = (n.C + 3) / 4 * 4;  // 16-byte voxel rows for the conv staging loads
        }
        n.buf = P.new_buffer((int64_t)n.D * n.H * n.W * n.cs);
    }
}

// ---------------- does conv_wfused serve the convolution?  (reads the storage of its input) ----------------------------------
void wf_pass(Planner& P) {
    if (!(P.kn.wfused && P.use_mfma && P.fuse)) return;
    for (auto& [i, L] : P.layers) {
        const Node& n = P.N[i];
        if (n.op != OP_CONV3D || n.ip[13] == ACT_SOFTMAX) continue;
        const Node& sn = P.N[L.f.src];
        TView iv = shape_of(sn);
        iv.cs = sn.cs; iv.coff = sn.coff;
        L.wf = conv_wf_view_ok(iv) && conv_wf_plan(iv, shape_of(n), L.g, sn.C, n.C, P.pool_mode(L.f), P.kn, &L.wfp);
    }
}

// ---------------- chunk-blocked layout ---------------------------------------------------------------------------------------
// chunk-blocked storage (TView::blk) for a tensor that is written by ONE pointwise / first-layer step and read by ONE
// conv_wfused step and by nothing else: that kernel reads 4-channel slices of whole frames, which are 16 bytes out of
// every voxel's channel row in the channels-last form (measured: 3.8x the tensor's bytes fetched from HBM) and one
// contiguous 16 KB run in the blocked form
void blocked_pass(Planner& P) {
    if (P.kn.wf_noblk) return;
    std::vector<Node>& N = P.N;
    for (auto& [i, L] : P.layers) {
        if (!L.wf) continue;
        const ConvFusion& f = L.f;
        const int src = f.src;
        Node& sn = N[src];
        if (src == P.m->input_node || src == P.m->output_node || !sn.materialised || sn.buf < 0) continue;
        if (sn.consumers.size() != 1 || sn.consumers[0] != (f.pre.empty() ? i : f.pre[0])) continue;
        if (sn.cs != sn.C || sn.coff != 0 || sn.C % 4) continue;
        int prod = -1, nprod = 0;
        for (auto& kv : P.layers) if (kv.second.f.last == src) { prod = kv.first; ++nprod; }
        if (nprod != 1) continue;
        const LayerPlan& pp = P.layers.at(prod);
        if (pp.wf) continue;                                        // (the producer itself runs on conv_wfused: channels-last stores only)
        if (!((pp.family == Kern::Pointwise && pp.pw.pool == 0) || (pp.family == Kern::First && pp.fp.nnb == 1))) continue;
        bool shared = false;                                        // nobody else may alias the buffer (Flatten / Identity views)
        for (int k = 0; k < (int)N.size(); ++k) if (k != src && N[k].buf == sn.buf && N[k].materialised) shared = true;
        if (shared) continue;
        sn.blk = 4;
    }
}

// ---------------- the kernel of every layer ----------------------------------------------------------------------------------
// the epilogue (own activation + absorbed elementwise chain) and the prologue of layer i
int build_epilogue(Planner& P, int i, LayerPlan& L) {
    const Node& n = P.N[i];
    const int own_act = n.op == OP_CONV3D ? n.ip[13] : n.ip[3];
    int rc;
    if (own_act == ACT_SOFTMAX) L.split_softmax = true;
    else if (own_act != ACT_LINEAR) add_act(&L.po, own_act, n.fp[0]);
    for (int x : L.f.post) if ((rc = add_post(P.m, &L.po, P.N[x]))) return rc < 0 ? rc : TH_EUNSUP;
    if (P.kn.no_pool_first) L.po.monotone = 0;   // A/B comparisons and tests: keep act/BN before the max-pool
    for (int x : L.f.pre) {
        const Node& pn = P.N[x];
        if (pn.op == OP_BN) { if ((rc = bn_affine(P.m, pn, &L.pre.scale, &L.pre.shift))) return rc; }
        else { L.pre.act = pn.ip[0]; L.pre.alpha = pn.fp[0]; }
    }
    return TH_OK;
}

// Dense node dn closes a GlobalAveragePooling3D -> Dense -> Softmax (the model output) tail within k_tail_dense's limits: F <= 2048 features
// (the pooled vectors of a workgroup's four frames in LDS), O <= 512 outputs (eight rounds of 64 lanes), no activation of its own
bool closes_dense_tail(const Planner& P, int dn) {
    const std::vector<Node>& N = P.N;
    const Node& d = N[dn];
    if (d.op != OP_DENSE || d.C > 512 || d.ip[3] != ACT_LINEAR || dn == P.m->output_node || d.consumers.size() != 1) return false;
    const Node& gp = N[d.in[0]];
    if (gp.op != OP_GAP || gp.C > 2048 || gp.consumers.size() != 1) return false;
    const Node& sm = N[d.consumers[0]];
    return sm.op == OP_ACT && sm.ip[0] == ACT_SOFTMAX && d.consumers[0] == P.m->output_node;
}

// in this order: wino -> wfs -> wf -> first5 -> first -> pointwise -> gl -> n16 / mfma -> direct.  After the chunk-blocked pass: the
// wfs and gl kernels read `blk`.
int choose_kernel(Planner& P, int i, LayerPlan& L) {
    th_model* m = P.m;
    if (int rc = build_epilogue(P, i, L)) return rc;
    const Node& n = P.N[i];
    const Node& sn = P.N[L.f.src];
    if (n.op == OP_DENSE) {
        if (sn.cs != sn.C || sn.coff != 0 || sn.D * sn.H * sn.W != 1) TH_FAIL(TH_EUNSUP, "%s: Dense needs a contiguous vector input", n.name.c_str());
        // TH_NO_TAIL_FUSE=1 is the A/B switch of k_tail_dense, which restates k_dense's fmaf chain: the tail's Dense stays on k_dense there,
        // so the two plans agree bit for bit at every F (k_dense_gemm sums F in four quarters)
        const bool tail_ab = P.kn.no_tail_fuse && closes_dense_tail(P, i);
        L.kind = P.kn.dense_gemm && !tail_ab && dense_gemm_ok(sn.C, n.C, m->bufs[sn.buf].floats_per_frame) ? Kern::DenseGemm : Kern::Dense;
        return TH_OK;
    }
    const ConvGeom& g = L.g;
    const TView iv = shape_of(sn), ov = shape_of(n);
    const int Cin = sn.C, Cout = n.C;
    if (P.kn.winograd && P.use_mfma && P.fuse && L.f.pool < 0 && !L.split_softmax &&
        conv_wino_plan(iv, ov, g, Cin, Cout, P.kn.winograd == 2 ? 7 : 9, P.kn.wino_split, P.kn, &L.wp))
        L.kind = Kern::Wino;
    else if (L.wf && conv_wfs_plan(L.wfp, m->view(L.f.src), L.pre, P.kn, &L.sp)) L.kind = Kern::WfSplit;
    else if (L.wf) L.kind = Kern::Wf;
    else if (L.family == Kern::First5 || L.family == Kern::First || L.family == Kern::Pointwise) L.kind = L.family;
    else if (conv_gl_wanted(P.kn.conv_gl, g, n.D * n.H * n.W) && L.f.pool < 0 && !sn.blk && !P.N[L.f.last].blk &&
             L.family != Kern::N16 &&                               // (the 16-wide kernel keeps its layers: 42 against 62 us on DenseCPD's 2^3 ones)
             conv_gl_ok(Cin, Cout, sn.cs, sn.coff, (int64_t)m->bufs[sn.buf].floats_per_frame))
        L.kind = Kern::Gl;
    else if (L.family == Kern::N16) L.kind = Kern::N16;
    else if (L.family == Kern::Mfma) {
        L.kind = Kern::Mfma;
        // heterogeneous Cout blocks: the last, mostly empty 128-column block on a narrower instantiation
        L.tailed = conv_mfma_plan_tail(iv, ov, g, Cin, Cout, L.mp.pool, L.mp, P.kn, &L.tp, &L.cout_main);
    } else L.kind = Kern::Direct;
    // the aposteriori case (21^3 frames, pool before a monotone chain) runs on the bf16 pipe with split operands
    if (L.kind == Kern::First) L.b3 = conv_first_b3_ok(L.fp, sn.D, sn.H, sn.W, Cin, std::min(Cout, 32), g, L.po);
    L.fp.ncu = L.np.ncu = L.wfp.ncu = L.sp.ncu = m->ncu;
    return TH_OK;
}

// ---------------- emission: one emitter per kernel family --------------------------------------------------------------------
// what a convolution's launch needs besides its plan: values only, so a step's run() may keep a copy (the device pointers of the
// tensors are bound at run time, th_model::view)
struct ConvArgs {
    th_model* M;
    int i, src, dst, Cin, Cout;
    ConvGeom g;
    const float* hw;       // Keras weights [kd][kh][kw][Cin][Cout], host
    const float* bias;     // device, or nullptr
    PreOp pre;
    PostOps po;
    TView in() const { return M->view(src); }
    TView out() const { return M->view(dst); }
    const Node& node(int k) const { return M->nodes[k]; }
};

// three or four steps, one kernel each.  `direct_flops` (the SURVEY §8d count of the direct form) stays with the GEMM step for
// the model total; the per-step `flops` are what the kernels really compute: the GEMM's own multiply-adds, nothing for the
// bandwidth-bound transforms (their bytes are V / M traffic)
int emit_wino(Planner& P, const ConvArgs& c, const LayerPlan& L, Step st) {
    th_model* M = c.M;
    std::vector<Node>& N = P.N;
    const ConvWinoPlan wp = L.wp;
    float* dw;
    if (int rc = upload_packed(M, wp.wpk_floats, [&](float* d) { conv_wino_pack_weights(wp, c.hw, d); }, &dw)) return rc;
    if (M->wino_v_buf < 0) { M->wino_v_buf = P.new_buffer(0); M->wino_m_buf = P.new_buffer(0); }
    int64_t& v_fpf = M->bufs[M->wino_v_buf].floats_per_frame;
    v_fpf = std::max(v_fpf, wp.v_fpf);
    M->bufs[M->wino_m_buf].floats_per_frame = std::max(M->bufs[M->wino_m_buf].floats_per_frame, wp.m_fpf);
    const Node& sn = N[c.src];
    const double direct = st.flops, act_bytes = st.bytes, in_floats = (double)sn.D * sn.H * sn.W * c.Cin, mf = (double)wp.m_fpf;
    const std::string name = N[c.i].name, pts = std::to_string(wp.P * wp.P);
    auto Vp = [M]() { const Buffer& b = M->bufs[M->wino_v_buf]; return b.dev + M->lane.off * b.floats_per_frame; };
    auto Mp = [M]() { const Buffer& b = M->bufs[M->wino_m_buf]; return b.dev + M->lane.off * b.floats_per_frame; };
    if (!P.wino_in_done.count(c.i))
        P.add_step(st.out_node, name + ": wino_in (25 voxels -> " + pts + " points per plane) [k_wino_in]", 4.0 * (in_floats + (double)wp.v_fpf),
                   [=](hipStream_t s, int64_t cnt) { return launch_wino_in(s, cnt, wp, c.in(), Vp(), c.pre); });
    st.flops = wp.gemm_flops;
    st.direct_flops = direct;
    // split GEMM: six bf16 piece products per fp32 multiply-add — what the bf16 matrix pipe issues
    st.exec_flops = wp.split ? 6.0 * wp.exec_flops : wp.exec_flops;
    st.bytes = 4.0 * ((double)wp.v_fpf + mf);
    st.label = name + ": " + wp.label + (wp.narrow ? " [k_wino_gemm_n32]" : wp.split ? " [k_wino_gemm_b3]" : " [k_wino_gemm]");
    st.run = [=](hipStream_t s, int64_t cnt) { return launch_wino_gemm(s, cnt, wp, Vp(), Mp(), dw); };
    P.add_step(st);
    const int dst = c.dst, Cout = c.Cout;
    // two Winograd layers in a row and nobody else reads the tensor between them: this layer's output transform feeds the
    // next layer's V directly (k_wino_mid) and the 5^3 activation is never written
    if (!P.kn.wino_nomid && dst != M->output_node && N[dst].consumers.size() == 1) {
        const int next = N[dst].consumers[0];
        const auto it = P.layers.find(next);
        const LayerPlan* nl = it == P.layers.end() ? nullptr : &it->second;
        if (nl && nl->kind == Kern::Wino && nl->f.src == dst && nl->f.pre.empty() && nl->wp.Cin == Cout) {
            v_fpf = std::max(v_fpf, nl->wp.v_fpf);
            P.add_step(st.out_node, name + ": wino_mid (" + pts + " points -> bias + epilogue -> " + pts + " points of " + N[next].name + ") [k_wino_mid]",
                       4.0 * (mf / wp.Coutp * Cout + (double)nl->wp.v_fpf),
                       [=](hipStream_t s, int64_t cnt) { return launch_wino_mid(s, cnt, wp, Mp(), Vp(), c.bias, c.po); });
            P.wino_in_done.insert(next);
            N[dst].materialised = false;        // th_model_fetch refuses it ("fused away")
            return TH_OK;
        }
    }
    // the layer's only reader is a GlobalAveragePooling3D (TIMED's 338-class head): the output transform pools
    // (k_wino_out<P, true>), neither the 5^3 activation nor the pooling kernel's pass over it exist
    int gp = -1;
    if (!P.kn.no_tail_fuse && dst != M->output_node) {
        int cur = dst;
        while (N[cur].consumers.size() == 1 && N[N[cur].consumers[0]].op == OP_IDENTITY && N[cur].consumers[0] != M->output_node)
            cur = N[cur].consumers[0];
        if (N[cur].consumers.size() == 1 && N[N[cur].consumers[0]].op == OP_GAP && N[N[cur].consumers[0]].materialised &&
            N[N[cur].consumers[0]].absorbed_by < 0) {
            bool single = true;          // every node of the chain has exactly one reader
            for (int k = dst; k != cur; k = N[k].consumers[0]) if (N[k].consumers.size() != 1) single = false;
            if (single) gp = N[cur].consumers[0];
        }
    }
    if (gp >= 0) {
        P.add_step(gp, name + ": wino_out + global_avg_pool (" + pts + " points -> bias + epilogue -> mean of the 125 voxels) [k_wino_out]",
                   4.0 * (mf / wp.Coutp * Cout + Cout),
                   [=](hipStream_t s, int64_t cnt) { return launch_wino_out(s, cnt, wp, Mp(), M->view(gp), c.bias, c.po, true); });
        for (int k = dst; ; k = N[k].consumers[0]) { N[k].materialised = false; if (N[k].consumers[0] == gp) break; }
        P.gap_done.insert(gp);
        return TH_OK;
    }
    P.add_step(st.out_node, name + ": wino_out (" + pts + " points -> 25 voxels per plane, bias + epilogue) [k_wino_out]",
               4.0 * (mf / wp.Coutp * Cout + (act_bytes / 4.0 - in_floats)),
               [=](hipStream_t s, int64_t cnt) { return launch_wino_out(s, cnt, wp, Mp(), c.out(), c.bias, c.po); });
    return TH_OK;
}

// the step's label: the layer's name, then the kernel's, with a remark when a tensor of the step is chunk-blocked
std::string conv_label(const ConvArgs& c, const std::string& kernel, bool in_blk, bool out_blk) {
    const std::string l = c.node(c.i).name + ": " + kernel;
    return in_blk ? label_note(l, " (input chunk-blocked)") : out_blk ? label_note(l, " (output chunk-blocked)") : l;
}

// the same algorithm as conv_wf on the bf16 pipe: both operands split exactly into three bf16 pieces (conv_wfsplit.hip)
int emit_wfs(const ConvArgs& c, const LayerPlan& L, Step& st) {
    const ConvWfsPlan sp = L.sp;
    float* dw;
    if (int rc = upload_packed(c.M, sp.wpk_floats, [&](float* d) { conv_wfs_pack_weights(sp, c.hw, d); }, &dw)) return rc;
    st.direct_flops = st.flops;
    st.flops = sp.own_flops;
    st.exec_flops = sp.exec_flops;
    st.label = conv_label(c, sp.label, c.node(c.src).blk, false);
    st.run = [=](hipStream_t s, int64_t cnt) { return launch_conv_wfs(s, cnt, sp, c.in(), c.out(), dw, c.bias, c.po); };
    return TH_OK;
}

// F(2,3)^2 in-plane with the whole transform domain in LDS: one step, one kernel (conv_wfused.hip)
int emit_wf(const ConvArgs& c, const LayerPlan& L, Step& st) {
    const ConvWfPlan fp = L.wfp;
    float* dw;
    if (int rc = upload_packed(c.M, fp.wpk_floats, [&](float* d) { conv_wf_pack_weights(fp, c.hw, d); }, &dw)) return rc;
    st.direct_flops = st.flops;
    st.flops = fp.own_flops;
    st.exec_flops = fp.exec_flops;
    st.label = conv_label(c, conv_wf_label(fp, c.pre), c.node(c.src).blk, false);
    st.run = [=](hipStream_t s, int64_t cnt) { return launch_conv_wf(s, cnt, fp, c.in(), c.out(), dw, c.bias, c.pre, c.po); };
    return TH_OK;
}

int emit_first5(const Planner& P, const ConvArgs& c, Step& st) {
    float* dw;
    if (int rc = upload_packed(c.M, conv_first5_wpk_floats(), [&](float* d) { conv_first5_pack_weights(c.Cin, c.Cout, c.hw, d); }, &dw))
        return rc;
    st.exec_flops = conv_first5_exec_flops();
    st.label = conv_label(c, conv_first5_label(), false, false);
    const ThKnobs* kn = &P.kn;
    st.run = [=](hipStream_t s, int64_t cnt) {
        return launch_conv_first5(s, cnt, kn, c.M->ncu, c.M->cur_in, c.M->cur_dtype, c.Cin, c.out(), c.Cout, dw, c.bias, c.po);
    };
    return TH_OK;
}

// the first layer on the caller's frames (conv_first.hip, conv_first_b3.hip): one launch per block of 32 output channels, each
// with its own weight columns, bias and per-channel epilogue vectors
int emit_first(const ConvArgs& c, const LayerPlan& L, Step& st) {
    const ConvFirstPlan fp = L.fp;
    const bool b3 = L.b3;
    if (fp.first_wino) {
        st.direct_flops = st.flops;
        st.flops = fp.own_flops;
    }
    st.exec_flops = b3 ? conv_first_b3_exec_flops() * fp.nnb : fp.exec_flops;
    st.label = conv_label(c, b3 ? conv_first_b3_label(fp.nnb) : conv_first_label(fp, c.Cin, c.po), false, c.node(c.dst).blk);
    if (fp.nnb > 1) st.label = label_note(st.label, (" x" + std::to_string(fp.nnb) + " passes of 32 columns").c_str());
    struct Pass { int c0, cn; float* dw; const float* bias; PostOps po; };
    std::vector<Pass> passes;
    const size_t ktaps = (size_t)c.g.kd * c.g.kh * c.g.kw * c.Cin;
    for (int c0 = 0; c0 < c.Cout; c0 += 32) {
        Pass ps{c0, std::min(32, c.Cout - c0), nullptr, c.bias ? c.bias + c0 : nullptr, post_from(c.po, c0)};
        const std::vector<float> wcol = weight_columns(c.hw, ktaps, c.Cout, c0, ps.cn);
        const int rc = upload_packed(c.M, b3 ? conv_first_b3_wpk_floats() : fp.wpk_floats, [&](float* d) {
            if (b3) conv_first_b3_pack_weights(c.Cin, ps.cn, wcol.data(), d);
            else if (fp.first_wino) conv_first_w_pack_weights(c.Cin, ps.cn, wcol.data(), d);
            else conv_first_pack_weights(c.Cin, ps.cn, wcol.data(), d);
        }, &ps.dw);
        if (rc) return rc;
        passes.push_back(ps);
    }
    const Node& sn = c.node(c.src);
    const int iD = sn.D, iH = sn.H, iW = sn.W;
    st.run = [=](hipStream_t s, int64_t cnt) {
        for (const Pass& ps : passes) {
            TView ov = c.out();
            if (passes.size() > 1) { ov.coff += ps.c0; ov.C = ps.cn; }
            th_model* M = c.M;
            const int r = b3 ? launch_conv_first_b3(s, cnt, fp, M->cur_in, M->cur_dtype, c.Cin, ov, ps.cn, ps.dw, ps.bias, ps.po)
                             : launch_conv_first(s, cnt, fp, M->cur_in, M->cur_dtype, iD, iH, iW, c.Cin, ov, c.g, ps.cn, ps.dw, ps.bias, ps.po);
            if (r) return r;
        }
        return (int)TH_OK;
    };
    return TH_OK;
}

int emit_pointwise(const ConvArgs& c, const LayerPlan& L, Step& st) {
    const ConvPwPlan pw = L.pw;
    float* dw;
    if (int rc = upload_packed(c.M, pw.wpk_floats, [&](float* d) { conv_pw_pack_weights(pw, c.Cin, c.Cout, c.hw, d); }, &dw)) return rc;
    const bool blk = c.node(c.dst).blk != 0;
    st.exec_flops = pw.exec_flops;
    st.label = conv_label(c, conv_pw_label(pw, c.in(), c.Cin, blk, c.po), false, blk);
    st.run = [=](hipStream_t s, int64_t cnt) { return launch_conv_pw(s, cnt, pw, c.in(), c.out(), c.Cin, c.Cout, dw, c.bias, c.pre, c.po); };
    return TH_OK;
}

// strided / few-outputs-per-frame layers: implicit GEMM with rows across the batch, operands from L2 (conv_gl.hip)
int emit_gl(const ConvArgs& c, Step& st) {
    float* dw;
    const size_t floats = conv_gl_wpk_floats(c.g, c.Cin, c.Cout);
    if (int rc = upload_packed(c.M, floats, [&](float* d) { conv_gl_pack_weights(c.g, c.Cin, c.Cout, c.hw, d); }, &dw)) return rc;
    const Node& n = c.node(c.i);
    st.exec_flops = conv_gl_exec_flops(c.g, c.Cin, c.Cout, n.D * n.H * n.W);
    st.label = conv_label(c, conv_gl_label(c.Cout), false, false);
    st.run = [=](hipStream_t s, int64_t cnt) { return launch_conv_gl(s, cnt, c.in(), c.out(), c.g, c.Cin, c.Cout, dw, c.bias, c.pre, c.po); };
    return TH_OK;
}

int emit_n16(const ConvArgs& c, const LayerPlan& L, Step& st) {
    const ConvN16Plan np = L.np;
    float* dw;
    if (int rc = upload_packed(c.M, np.wpk_floats, [&](float* d) { conv_n16_pack_weights(np, c.Cin, c.Cout, c.hw, d); }, &dw)) return rc;
    st.exec_flops = np.exec_flops;
    st.label = conv_label(c, np.label, false, false);
    st.run = [=](hipStream_t s, int64_t cnt) { return launch_conv_n16(s, cnt, np, c.in(), c.out(), c.g, c.Cin, c.Cout, dw, c.bias, c.pre, c.po); };
    return TH_OK;
}

int emit_mfma(const ConvArgs& c, const LayerPlan& L, Step& st) {
    ConvMfmaPlan mp = L.mp;
    float *dw, *dwt;
    int rc;
    if (!L.tailed) {
        if ((rc = upload_packed(c.M, mp.wpk_floats, [&](float* d) { conv_mfma_pack_weights(mp, c.g, c.Cin, c.Cout, c.hw, d); }, &dw))) return rc;
        st.exec_flops = mp.exec_flops;
        st.label = conv_label(c, mp.label, false, false);
        st.run = [=](hipStream_t s, int64_t cnt) { return launch_conv_mfma(s, cnt, mp, c.in(), c.out(), c.g, c.Cin, c.Cout, dw, c.bias, c.pre, c.po); };
        return TH_OK;
    }
    // the last Cout block on the narrower `tp`: output channels [cout_main, Cout)
    const ConvMfmaPlan tp = L.tp;
    const int cout_main = L.cout_main, cout_tail = c.Cout - cout_main;
    const size_t ktaps = (size_t)c.g.kd * c.g.kh * c.g.kw * c.Cin;
    const std::vector<float> wm = weight_columns(c.hw, ktaps, c.Cout, 0, cout_main), wt = weight_columns(c.hw, ktaps, c.Cout, cout_main, cout_tail);
    mp.nnb -= 1;
    mp.exec_flops *= (double)mp.nnb / (mp.nnb + 1);
    mp.wpk_floats = mp.wpk_floats / (mp.nnb + 1) * mp.nnb;
    if ((rc = upload_packed(c.M, mp.wpk_floats, [&](float* d) { conv_mfma_pack_weights(mp, c.g, c.Cin, cout_main, wm.data(), d); }, &dw)) ||
        (rc = upload_packed(c.M, tp.wpk_floats, [&](float* d) { conv_mfma_pack_weights(tp, c.g, c.Cin, cout_tail, wt.data(), d); }, &dwt)))
        return rc;
    const PostOps pot = post_from(c.po, cout_main);
    const float* bias_t = c.bias ? c.bias + cout_main : nullptr;
    st.exec_flops = mp.exec_flops + tp.exec_flops;
    st.label = conv_label(c, conv_mfma_tailed_label(L.mp, tp), false, false);
    st.run = [=](hipStream_t s, int64_t cnt) {
        int r1 = launch_conv_mfma(s, cnt, mp, c.in(), c.out(), c.g, c.Cin, cout_main, dw, c.bias, c.pre, c.po);
        if (r1) return r1;
        TView ot = c.out();
        ot.coff += cout_main;
        return launch_conv_mfma(s, cnt, tp, c.in(), ot, c.g, c.Cin, cout_tail, dwt, bias_t, c.pre, pot);
    };
    return TH_OK;
}

int emit_direct(const ConvArgs& c, Step& st) {
    float* dw;
    if (int rc = upload(c.M, c.hw, (size_t)c.g.kd * c.g.kh * c.g.kw * c.Cin * c.Cout, &dw)) return rc;
    st.exec_flops = st.flops;
    st.label = conv_label(c, "conv3d_direct", false, false);
    st.run = [=](hipStream_t s, int64_t cnt) { return launch_conv3d_direct(s, cnt, c.in(), c.out(), c.g, dw, c.bias, c.pre, c.po); };
    return TH_OK;
}

int emit_dense(const ConvArgs& c, const LayerPlan& L, Step& st) {
    const int F = c.Cin, O = c.Cout;
    if (c.M->blob_count[c.node(c.i).w[0]] != (size_t)F * O) TH_FAIL(TH_EIO, "%s: kernel size mismatch", c.node(c.i).name.c_str());
    float* dw;
    if (int rc = upload(c.M, c.hw, (size_t)F * O, &dw)) return rc;
    st.flops = st.exec_flops = 2.0 * F * O;
    st.bytes = 4.0 * (F + O);
    if (L.kind == Kern::DenseGemm) {
        st.label = conv_label(c, "dense as a batch GEMM, 16 frames x all outputs per workgroup, F in four quarters (16x16x4 fp32 MFMA) [k_dense_gemm]",
                              false, false);
        st.run = [=](hipStream_t s, int64_t cnt) { return launch_dense_gemm(s, cnt, c.in(), c.out(), dw, c.bias, c.po); };
    } else {
        st.label = conv_label(c, "dense", false, false);
        st.run = [=](hipStream_t s, int64_t cnt) { return launch_dense(s, cnt, c.in(), c.out(), dw, c.bias, c.po); };
    }
    return TH_OK;
}

// a 3x3x3 stride-1 layer that stays on a direct kernel says why no minimal-filtering form took it (tools/plan_report.py)
void note_direct_form(const Planner& P, const ConvArgs& c, const LayerPlan& L, Step& st) {
    const ConvGeom& g = c.g;
    const Node& sn = c.node(c.src);
    const bool k333 = g.kd == 3 && g.kh == 3 && g.kw == 3 && g.sd == 1 && g.sh == 1 && g.sw == 1 && g.dd == 1 && g.dh == 1 && g.dw == 1;
    if (!k333 || fast_form(L)) return;
    std::string why;
    const bool same = g.pz == 1 && g.py == 1 && g.px == 1;
    if (!P.use_mfma || !P.fuse) why = "load flags select the direct kernels";
    else if (!same) why = "'valid' padding (the Cook-Toom forms are built for 'same')";
    else if (c.src == P.m->input_node && sn.C <= 8 && c.Cout <= 32) why = P.kn.first_wino ? "odd computed width" : "TH_FIRST_WINO=0";
    else if (sn.D == 5 && sn.H == 5 && sn.W == 5) {
        if (!P.kn.winograd) why = "TH_WINOGRAD=0";
        else if (L.f.pool >= 0) why = "a pooling layer is fused behind it";
        else if (sn.C < 32) why = "Cin < 32";
        else if (c.Cout < 64) why = "Cout < 64 (a 128-column GEMM block would run mostly empty)";
        else why = "softmax fused into the layer";
    } else if (sn.H % 2 == 0 && sn.W % 2 == 0 && sn.D * (sn.H / 2) * (sn.W / 2) <= 250) {
        if (!P.kn.wfused) why = "TH_WFUSED=0";
        else if (sn.C < 16 || sn.C % 4) why = "Cin < 16 or not a multiple of 4";
        else if (!(sn.D == 10 && sn.H == 10 && sn.W == 10)) why = "conv_wf is instantiated for 10^3 volumes only";
        else why = "input view is not 16-byte aligned";
    } else why = "no minimal-filtering kernel for a " + std::to_string(sn.D) + "x" + std::to_string(sn.H) + "x" + std::to_string(sn.W) +
                 " volume (conv_wf: 10^3, conv_wino: 5^3)";
    st.label = label_note(st.label, (" (direct form: " + why + ")").c_str());
}

// the step(s) of Conv3D / Dense layer i
int emit_layer(Planner& P, int i) {
    th_model* M = P.m;
    const Node& n = P.N[i];
    const LayerPlan& L = P.layers.at(i);
    const Node& sn = P.N[L.f.src];
    const Node& dn = P.N[L.f.last];
    const float* hw = n.w[0] >= 0 ? M->blob_host[n.w[0]] : nullptr;
    if (!hw) TH_FAIL(TH_EIO, "%s: missing kernel", n.name.c_str());
    float* bias = nullptr;
    int rc = TH_OK;
    if ((n.op == OP_CONV3D ? n.ip[12] : n.ip[2]) != 0) {
        if (n.w[1] < 0) TH_FAIL(TH_EIO, "%s: missing bias", n.name.c_str());
        if ((rc = upload(M, M->blob_host[n.w[1]], M->blob_count[n.w[1]], &bias))) return rc;
    }
    const ConvGeom& g = L.g;
    const ConvArgs c{M, i, L.f.src, L.f.last, sn.C, n.C, g, hw, bias, L.pre, L.po};
    Step st;
    st.out_node = c.dst;
    st.fast = fast_form(L);
    if (n.op == OP_CONV3D) {
        if (M->blob_count[n.w[0]] != (size_t)g.kd * g.kh * g.kw * c.Cin * c.Cout) TH_FAIL(TH_EIO, "%s: kernel size mismatch", n.name.c_str());
        st.flops = 2.0 * n.D * n.H * n.W * (double)g.kd * g.kh * g.kw * c.Cin * c.Cout;
        st.bytes = 4.0 * ((double)sn.D * sn.H * sn.W * c.Cin + (double)dn.D * dn.H * dn.W * dn.C);
    }
    switch (L.kind) {
        case Kern::Wino: return emit_wino(P, c, L, st);
        case Kern::WfSplit: rc = emit_wfs(c, L, st); break;
        case Kern::Wf: rc = emit_wf(c, L, st); break;
        case Kern::First5: rc = emit_first5(P, c, st); break;
        case Kern::First: rc = emit_first(c, L, st); break;
        case Kern::Pointwise: rc = emit_pointwise(c, L, st); break;
        case Kern::Gl: rc = emit_gl(c, st); break;
        case Kern::N16: rc = emit_n16(c, L, st); break;
        case Kern::Mfma: rc = emit_mfma(c, L, st); break;
        case Kern::DenseGemm: case Kern::Dense: rc = emit_dense(c, L, st); break;
        default: rc = emit_direct(c, st); break;
    }
    if (rc) return rc;
    if (n.op == OP_CONV3D) note_direct_form(P, c, L, st);
    P.add_step(st);
    if (L.split_softmax) {
        const bool final_softmax = c.dst == M->output_node;
        P.add_step(c.dst, n.name + ": softmax (layer activation)", 0,
                   [=](hipStream_t s, int64_t cnt) { return launch_softmax(s, cnt, c.out(), c.out()); }).is_final_softmax = final_softmax;
        if (final_softmax) M->logits_node = c.dst;
    }
    return TH_OK;
}

// DenseCPD's tail [BatchNormalization / activation]* -> GlobalAveragePooling3D -> Dense -> Softmax (the model output) as ONE
// launch, one wavefront per frame (k_tail_dense).  Called at the first node of the chain; fills *st and returns 1 when the
// pattern holds (0: no, < 0: error).  The pooled vector and the logits are still written to their nodes' buffers; the
// elementwise nodes in front of the pooling are fused away.
int try_dense_tail(Planner& P, int first, Step* st) {
    th_model* M = P.m;
    std::vector<Node>& N = P.N;
    if (!P.fuse || P.kn.no_tail_fuse) return 0;
    std::vector<int> chain;
    int j = first;
    while ((N[j].op == OP_BN || (N[j].op == OP_ACT && N[j].ip[0] != ACT_SOFTMAX)) && (int)chain.size() < TH_MAX_POST) {
        if (N[j].absorbed_by >= 0 || !N[j].materialised || N[j].consumers.size() != 1 || j == M->output_node) return 0;
        chain.push_back(j);
        j = N[j].consumers[0];
    }
    const int gp = j;
    if (N[gp].op != OP_GAP || P.gap_done.count(gp) || N[gp].absorbed_by >= 0 || !N[gp].materialised || N[gp].consumers.size() != 1 ||
        gp == M->output_node)
        return 0;
    const int dn = N[gp].consumers[0];
    // (Dense(activation='softmax') keeps its two steps: logits and probabilities share the node there, and a TH_PREDICT_LOGITS
    // call drops the in-place softmax step)
    if (!closes_dense_tail(P, dn) || !P.layers.count(dn) || N[dn].w[0] < 0) return 0;
    const ConvFusion& f = P.layers.at(dn).f;
    if (f.src != gp || !f.pre.empty() || !f.post.empty() || f.pool >= 0 || f.last != dn || !N[dn].materialised) return 0;
    const int sm = N[dn].consumers[0];                  // node that holds the probabilities
    if (N[sm].absorbed_by >= 0 || !N[sm].materialised) return 0;
    const int src = N[chain.empty() ? gp : chain[0]].in[0];
    if (N[src].blk || !N[src].materialised || N[src].buf < 0) return 0;
    const Node& gn = N[gp];
    if (gn.cs != gn.C || gn.coff != 0) return 0;         // k_dense's contract: a contiguous feature vector
    PostOps pre, post;
    int rc;
    for (int x : chain) if ((rc = add_post(M, &pre, N[x]))) return rc < 0 ? rc : 0;
    const int F = gn.C, O = N[dn].C;
    if (M->blob_count[N[dn].w[0]] != (size_t)F * O) return 0;   // (the Dense case reports the mismatch)
    float *dw = nullptr, *dbias = nullptr;
    if ((rc = upload(M, M->blob_host[N[dn].w[0]], (size_t)F * O, &dw))) return rc;
    if (N[dn].ip[2]) {
        if (N[dn].w[1] < 0) return 0;
        if ((rc = upload(M, M->blob_host[N[dn].w[1]], M->blob_count[N[dn].w[1]], &dbias))) return rc;
    }
    const int V = N[src].D * N[src].H * N[src].W;
    st->out_node = sm;
    st->flops = st->exec_flops = 2.0 * F * O;
    st->bytes = 4.0 * ((double)V * N[src].C + F + 2.0 * O);
    st->label = N[first].name + ": " + (chain.empty() ? "" : std::to_string(chain.size()) + " elementwise + ") +
                "global_avg_pool + dense + softmax [k_tail_dense]";
    st->run = [=](hipStream_t s, int64_t cnt) {
        return launch_tail_dense(s, cnt, M->view(src), pre, M->view(gp), M->view(dn), M->view(sm), dw, dbias, post, 1);
    };
    M->logits_node = dn;
    for (int x : chain) { P.tail_done.insert(x); N[x].materialised = false; }   // th_model_fetch refuses them ("fused away")
    P.tail_done.insert(gp); P.tail_done.insert(dn); P.tail_done.insert(sm);
    P.tail_done.erase(first);
    return 1;
}

// GlobalAveragePooling3D / GlobalMaxPooling3D node i, with the tails fused into it
int emit_global_pool(Planner& P, int i) {
    th_model* M = P.m;
    std::vector<Node>& N = P.N;
    const Node& n = N[i];
    const int src = n.in[0];
    const int is_max = n.op == OP_GMP;
    // the model's final softmax right behind the pooling, when it is nothing else's input
    const int sm = n.consumers.size() == 1 ? n.consumers[0] : -1;
    const bool softmax_out = sm >= 0 && N[sm].op == OP_ACT && N[sm].ip[0] == ACT_SOFTMAX && sm == M->output_node && N[sm].absorbed_by < 0 &&
                             N[sm].materialised;
    Step st;
    st.out_node = i;
    if (P.gap_done.count(i)) {
        // pooled by k_wino_out<P, true>; what is left of the tail is the softmax over the pooled logits
        if (!softmax_out) return TH_OK;
        st.out_node = sm;
        st.label = N[sm].name + ": softmax (logits pooled by the output transform) [k_softmax]";
        st.is_final_softmax = true;
        st.bytes = 8.0 * n.C;
        st.run = [=](hipStream_t s, int64_t cnt) { return launch_softmax(s, cnt, M->view(i), M->view(sm)); };
        M->logits_node = i;
        P.fused_tail = sm;
    } else if (int rc = is_max ? 0 : try_dense_tail(P, i, &st)) {
        if (rc < 0) return rc;
    } else if (!is_max && P.fuse && softmax_out && n.C <= 512 && !P.kn.no_tail_fuse && n.materialised) {
        // TIMED's tail GlobalAveragePooling3D -> Softmax (the model output): one launch, one wavefront per frame
        st.label = n.name + ": global_avg_pool + softmax [k_gap_softmax]";
        st.bytes = 4.0 * ((double)N[src].D * N[src].H * N[src].W * N[src].C + 2.0 * n.C);
        st.run = [=](hipStream_t s, int64_t cnt) { return launch_gap_softmax(s, cnt, M->view(src), M->view(i), M->view(sm)); };
        M->logits_node = i;
        P.fused_tail = sm;
    } else {
        st.label = n.name + (is_max ? ": global_max_pool" : ": global_avg_pool");
        st.bytes = 4.0 * N[src].D * N[src].H * N[src].W * N[src].C;
        st.run = [=](hipStream_t s, int64_t cnt) { return launch_global_pool(s, cnt, M->view(src), M->view(i), is_max); };
    }
    P.add_step(st);
    return TH_OK;
}

// the step(s) of node i that is not a Conv3D / Dense layer
int emit_node(Planner& P, int i) {
    th_model* M = P.m;
    std::vector<Node>& N = P.N;
    const Node& n = N[i];
    Step st;
    st.out_node = i;
    switch (n.op) {
        case OP_INPUT: return TH_OK;          // the convert step is issued by predict() itself (it needs the caller's pointer/dtype)
        case OP_BN:
        case OP_ACT: {
            const int src = n.in[0];
            if (i == P.fused_tail) return TH_OK;      // computed by the k_gap_softmax step of its input
            if (int rc = try_dense_tail(P, i, &st)) { if (rc < 0) return rc; break; }
            if (n.op == OP_ACT && n.ip[0] == ACT_SOFTMAX) {
                st.label = n.name + ": softmax";
                st.is_final_softmax = i == M->output_node;
                if (st.is_final_softmax) M->logits_node = src;
                st.run = [=](hipStream_t s, int64_t cnt) { return launch_softmax(s, cnt, M->view(src), M->view(i)); };
            } else {
                PostOps po;
                int rc = add_post(M, &po, n);
                if (rc) return rc < 0 ? rc : TH_EUNSUP;
                st.label = n.name + (n.op == OP_BN ? ": batchnorm" : ": activation");
                st.run = [=](hipStream_t s, int64_t cnt) { return launch_eltwise(s, cnt, M->view(src), M->view(i), po); };
            }
            st.bytes = 8.0 * n.D * n.H * n.W * n.C;
            break;
        }
        case OP_MAXPOOL:
        case OP_AVGPOOL: {
            const int src = n.in[0];
            const Node& sn = N[src];
            ConvGeom g{};
            g.kd = n.ip[0]; g.kh = n.ip[1]; g.kw = n.ip[2]; g.sd = n.ip[3]; g.sh = n.ip[4]; g.sw = n.ip[5];
            g.dd = g.dh = g.dw = 1;
            if (n.ip[6]) {
                keras_same_pad(sn.D, g.kd, g.sd, 1, &g.pz);
                keras_same_pad(sn.H, g.kh, g.sh, 1, &g.py);
                keras_same_pad(sn.W, g.kw, g.sw, 1, &g.px);
            }
            const int is_max = n.op == OP_MAXPOOL;
            st.label = n.name + (is_max ? ": maxpool3d" : ": avgpool3d");
            st.bytes = 4.0 * ((double)sn.D * sn.H * sn.W * sn.C + (double)n.D * n.H * n.W * n.C);
            st.run = [=](hipStream_t s, int64_t cnt) { return launch_pool3d(s, cnt, M->view(src), M->view(i), g, is_max); };
            break;
        }
        case OP_GAP:
        case OP_GMP: return emit_global_pool(P, i);
        case OP_FLATTEN:
        case OP_IDENTITY: {
            const int src = n.in[0];
            if (n.buf == N[src].buf && n.coff == 0) return TH_OK;  // alias, nothing to do
            // gather a channel-sliced tensor into a dense [V*C] vector
            st.label = n.name + ": flatten(copy)";
            st.run = [=](hipStream_t s, int64_t cnt) {
                TView o = M->view(src);  // same shape, destination is dense
                o.p = M->bufs[M->nodes[i].buf].dev; o.cs = o.C; o.coff = 0; o.fs = M->bufs[M->nodes[i].buf].floats_per_frame;
                return launch_copy(s, cnt, M->view(src), o);
            };
            break;
        }
        case OP_CONCAT: {
            int off = 0;
            for (size_t k = 0; k < n.in.size(); ++k) {
                const int src = n.in[k];
                const int o = off;
                off += N[src].C;
                if (!P.concat_copy[i * kMaxIn + k]) continue;
                P.add_step(i, n.name + ": concat(copy " + N[src].name + ")", 8.0 * N[src].D * N[src].H * N[src].W * N[src].C,
                           [=](hipStream_t s, int64_t cnt) {
                               TView d = M->view(i);
                               d.coff += o;
                               d.C = M->nodes[src].C;
                               return launch_copy(s, cnt, M->view(src), d);
                           });
            }
            return TH_OK;
        }
        case OP_ADD: {
            if (n.in.size() < 2) TH_FAIL(TH_EUNSUP, "%s: Add needs >= 2 inputs", n.name.c_str());
            for (size_t k = 1; k < n.in.size(); ++k) {
                const int a = k == 1 ? n.in[0] : i, b = n.in[k];
                P.add_step(i, n.name + ": add", 12.0 * n.D * n.H * n.W * n.C,
                           [=](hipStream_t s, int64_t cnt) { return launch_add(s, cnt, M->view(a), M->view(b), M->view(i)); });
            }
            return TH_OK;
        }
        default:
            TH_FAIL(TH_EUNSUP, "node %s: op %d not supported", n.name.c_str(), n.op);
    }
    P.add_step(st);
    return TH_OK;
}

}  // namespace

// the load-time planner: the model's graph -> m->steps, a short list of launches
int th_rt::plan(th_model* m) {
    Planner P(m);
    fusion_pass(P);
    storage_pass(P);
    wf_pass(P);
    blocked_pass(P);
    for (auto& [i, L] : P.layers)
        if (int rc = choose_kernel(P, i, L)) return rc;
    for (int i = 0; i < (int)P.N.size(); ++i) {
        if (!(P.layers.count(i) || P.N[i].absorbed_by < 0) || P.tail_done.count(i)) continue;
        const int rc = P.layers.count(i) ? emit_layer(P, i) : emit_node(P, i);
        if (rc) return rc;
    }
    for (const Step& s : m->steps) { m->algo_flops += s.direct_flops >= 0 ? s.direct_flops : s.flops; m->exec_flops += s.exec_flops; }
    return TH_OK;
}

// ---- the brick kernels' rule: choose_family's decision, and its export for tests (include/timed_hip.h) -----------------------
int conv_brick_plan(const TView& in, const TView& oc, const ConvGeom& g, int Cin, int Cout, int pool, const ThKnobs& kn,
                    ConvN16Plan* np, ConvMfmaPlan* mp) {
    return conv_n16_plan(in, oc, g, Cin, Cout, pool, kn, np) ? 1 : conv_mfma_plan(in, oc, g, Cin, Cout, pool, kn, mp) ? 2 : 0;
}

// the plan label of a kd x kh x kw convolution, Cin -> Cout, on a D x H x W volume with this pool value (0 none, 1 max, 2 avg) under
// the default knobs: conv_brick_plan, and for a k_conv_mfma plan conv_mfma_plan_tail, joined as the step label joins them; "" when
// neither kernel plans the layer.  in_cs (<= 0: a dense tensor of its own) and in_coff describe the input view.
extern "C" int th_conv_brick_pick(int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, const int stride[3], const int dilation[3],
                                  int same, int pool, int in_cs, int in_coff, char* buf, size_t len) {
    if (!buf || !len || !stride || !dilation || pool < 0 || pool > 2 || D < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || kd < 1 || kh < 1 ||
        kw < 1 || stride[0] < 1 || stride[1] < 1 || stride[2] < 1 || dilation[0] < 1 || dilation[1] < 1 || dilation[2] < 1)
        TH_FAIL(TH_EINVAL, "th_conv_brick_pick: bad arguments");
    static const ThKnobs kn;
    Node src, cv;
    src.D = D; src.H = H; src.W = W; src.C = Cin;
    const int k[3] = {kd, kh, kw}, ext[3] = {D, H, W};
    int out[3];
    for (int a = 0; a < 3; ++a) {
        const int ke = (k[a] - 1) * dilation[a] + 1;
        out[a] = same ? (ext[a] + stride[a] - 1) / stride[a] : (ext[a] - ke) / stride[a] + 1;
        if (ext[a] < ke && !same) out[a] = 0;
        cv.ip[a] = k[a]; cv.ip[3 + a] = stride[a]; cv.ip[6 + a] = dilation[a];
    }
    cv.ip[9] = same ? 1 : 0;
    cv.D = out[0]; cv.H = out[1]; cv.W = out[2]; cv.C = Cout;
    buf[0] = 0;
    if (out[0] < 1 || out[1] < 1 || out[2] < 1) return TH_OK;
    const ConvGeom g = conv_geom(cv, src);
    TView iv = shape_of(src);
    const TView ov = shape_of(cv);
    if (in_cs > 0) { iv.cs = in_cs; iv.coff = in_coff; iv.fs = (int64_t)iv.V() * in_cs; }
    ConvN16Plan np;
    ConvMfmaPlan mp, tp;
    int cout_main = 0;
    const int b = conv_brick_plan(iv, ov, g, Cin, Cout, pool, kn, &np, &mp);
    std::string label;
    if (b == 1) label = np.label;
    else if (b == 2) label = conv_mfma_plan_tail(iv, ov, g, Cin, Cout, mp.pool, mp, kn, &tp, &cout_main) ? conv_mfma_tailed_label(mp, tp) : mp.label;
    if (label.size() + 1 > len) TH_FAIL(TH_EINVAL, "th_conv_brick_pick: %zu bytes needed", label.size() + 1);
    std::memcpy(buf, label.c_str(), label.size() + 1);
    return TH_OK;
}

// every compiled instantiation of the two brick kernels, one name per line: generated from the dispatch tables of conv_mfma.hip and conv_n16.hip
extern "C" int th_conv_brick_kernels(char* buf, size_t len) {
    if (!buf || !len) TH_FAIL(TH_EINVAL, "th_conv_brick_kernels: bad arguments");
    std::string all;
    conv_mfma_kernel_names(&all);
    conv_n16_kernel_names(&all);
    if (all.size() + 1 > len) TH_FAIL(TH_EINVAL, "th_conv_brick_kernels: %zu bytes needed", all.size() + 1);
    std::memcpy(buf, all.c_str(), all.size() + 1);
    return TH_OK;
}
