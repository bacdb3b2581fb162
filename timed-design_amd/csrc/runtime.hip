// Model runtime: pack loader, layer-graph planner (fusion + zero-copy concat), executor, C ABI.
//
// Replaces, behind include/timed_hip.h:
//   tf.keras.models.load_model(path)      reference predict.py:121  -> th_model_load
//   frame_model.predict(X_batch)          reference predict.py:142  -> th_predict / th_predict_device
// The reference hands the network to TensorFlow as an opaque graph; here the graph is planned once
// at load time into a short list of launches:
//   * Conv3D + bias + {ELU/ReLU, BatchNorm}* + MaxPool/AvgPool(2) -> ONE fused MFMA kernel
//     (conv_mfma.hip); a BN->ReLU in FRONT of a conv (DenseNet/DenseCPD pre-activation) becomes the
//     kernel's staging prologue;
//   * Concatenate is zero-copy: producers write straight into a channel slice of the concat
//     buffer (nested concats collapse into one buffer per dense block);
//   * everything else runs on the generic kernels (kernels_generic.hip).
// Activations live in HBM as channels-last fp32, one arena per tensor sized for `chunk` frames.
#include "common.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <set>

#include <dlfcn.h>
#include <sys/stat.h>
#include <unistd.h>

// ---- errors ---------------------------------------------------------------------------------
static thread_local char g_err[1024] = "";
void th_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

// ---- A/B and test knobs (ThKnobs, common.h) ---------------------------------------------------------------------------------
int th_knobs_read(ThKnobs* k) {
    *k = ThKnobs();
    std::string& nd = k->nondefault;
    auto note = [&](const char* name, const char* v) { nd += (nd.empty() ? "" : " "); nd += name; nd += "="; nd += v; };
    auto num = [&](const char* name, int* dst, int lo, int hi) {          // integer knob, clamped; listed when it changes the default
        const char* e = getenv(name);
        if (!e) return;
        const int v = std::max(lo, std::min(hi, atoi(e)));
        if (v != *dst) note(name, e);
        *dst = v;
    };
    auto flag = [&](const char* name, int* dst) {                        // on / off knob: unset, empty or 0 = off, like the num() knobs
        const char* e = getenv(name);                                    // (NAME=0 used to switch these ON by presence)
        if (e && *e && atoi(e) != 0) { *dst = 1; note(name, e); }
    };
    const char* refused = nullptr;      // a knock-out variable that is set where no knock-out exists: whole kernels must not be timed as knocked out
#if TH_KNOCKOUTS
#define KNOCK(name, field) num(name, &k->field, 0, 1 << 20)
#else
    auto refuse = [&](const char* name) { const char* e = getenv(name); if (!refused && e && atoi(e) != 0) refused = name; };
#define KNOCK(name, field) refuse(name)
#endif
    num("TH_WINOGRAD", &k->winograd, 0, 2);
    num("TH_WINO_SPLIT", &k->wino_split, 0, 1);
    num("TH_WFUSED", &k->wfused, 0, 1);
    num("TH_WF_SPLIT", &k->wf_split, 0, 1);
    if (const char* e = getenv("TH_LANES")) { k->lanes = atoi(e) == 2 ? 2 : 1; if (k->lanes != 1) note("TH_LANES", e); }
    num("TH_LANE_LAG", &k->lane_lag, 0, 1 << 20);
    num("TH_GUARD", &k->guard, 0, 2);
    num("TH_FIRST_WINO", &k->first_wino, 0, 1);
    num("TH_FIRST_SPLIT", &k->first_split, 0, 1);
    num("TH_FIRST_INT", &k->first_int, 0, 1);
    num("TH_DENSE_GEMM", &k->dense_gemm, 0, 1);
    num("TH_CONV_GL", &k->conv_gl, 0, 2);
    KNOCK("TH_FIRST_DBG", first_dbg);
    flag("TH_NO_POOL_FIRST", &k->no_pool_first);
    flag("TH_NO_TAIL_FUSE", &k->no_tail_fuse);
    flag("TH_CONV_NOGEO", &k->conv_nogeo);
    flag("TH_N16_NOGEO", &k->n16_nogeo);
    flag("TH_CONV_NOXC", &k->conv_noxc);
    flag("TH_CONV_NOTAIL", &k->conv_notail);
    flag("TH_CONV_NOZMAJOR", &k->conv_nozmajor);
    flag("TH_CONV_NOCOMPACT", &k->conv_nocompact);
    flag("TH_CONV_NOPW", &k->conv_nopw);
    if (const char* e = getenv("TH_CONV_BMODE")) {
        k->conv_bmode = !std::strcmp(e, "dbuf") ? 1 : !std::strcmp(e, "stream8") ? 2 : !std::strcmp(e, "no16") ? 3 : 0;
        if (k->conv_bmode) note("TH_CONV_BMODE", e);
    }
    KNOCK("TH_CONV_DBG", conv_dbg);
    num("TH_N16_RESIDENT", &k->n16_resident, 0, 1 << 20);
    flag("TH_PW_NOPIPE", &k->pw_nopipe);
    flag("TH_PW_NOEPI", &k->pw_noepi);
    KNOCK("TH_PW_DBG", pw_dbg);
    num("TH_WF_RESIDENT", &k->wf_resident, 0, 1 << 20);
    KNOCK("TH_WF_DBG", wf_dbg);
    num("TH_WF_NOBLK", &k->wf_noblk, 0, 1);
    if (const char* e = getenv("TH_WINO_PIECE")) { k->wino_piece = std::max(0ll, atoll(e)); if (k->wino_piece) note("TH_WINO_PIECE", e); }
    KNOCK("TH_WINO_DBG", wino_dbg);
    num("TH_WINO_B3VAR", &k->wino_b3var, 0, 2);
    num("TH_WINO_NOMID", &k->wino_nomid, 0, 1);
#undef KNOCK
    if (refused)
        TH_FAIL(TH_EINVAL, "%s is set, but this library has no timing knock-outs: build the knock-out library "
                           "(tools/build_knockouts.py) and load it through TIMED_HIP_LIB", refused);
    return TH_OK;
}

// ---- device block cache ---------------------------------------------------------------------------------------------------
// predict.py loads and frees a model per call (the reference does: predict.py:114-121); a TIMED handle is ~50 device blocks —
// weights, activation arenas, rings — and hipFree synchronises the device each time: 13 ms per close, 10 ms per load.  Blocks a
// model gives back are kept here (exact-size reuse, at most kCacheBytes per process) and returned to HIP by th_dev_trim or when
// the cap is reached.  Callers synchronise the streams that used a block before they release it.
namespace {
struct DevCache {
    std::mutex mu;
    struct Blk { void* p; uint64_t stamp; };
    std::multimap<std::pair<int, size_t>, Blk> free_blocks;     // (device, bytes) -> block, with the time it was parked
    std::map<void*, std::pair<int, size_t>> live;               // blocks handed out
    std::map<int, size_t> cached_bytes;                         // per device
    std::map<int, size_t> cap_bytes;                            // per device: min(kCacheBytes, an eighth of the device's memory)
    uint64_t clock = 0;
    static constexpr size_t kCacheBytes = 24ull << 30;
    static constexpr size_t kCacheBlocks = 1024;
};
DevCache g_cache;

// the cap of `device` (lock held): the fixed 24 GB of round 4 is more than a small card has — an eighth of the device's memory
size_t cache_cap_locked(int device) {
    auto it = g_cache.cap_bytes.find(device);
    if (it != g_cache.cap_bytes.end()) return it->second;
    size_t cap = DevCache::kCacheBytes, free_b = 0, total_b = 0;
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && (cur == device || hipSetDevice(device) == hipSuccess)) {
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && total_b) cap = std::min(cap, total_b / 8);
        if (cur >= 0 && cur != device) (void)hipSetDevice(cur);
    }
    (void)hipGetLastError();
    g_cache.cap_bytes[device] = cap;
    return cap;
}

int cached_malloc(void** out, size_t bytes, int device) {
    if (!bytes) bytes = 4;
    {
        std::lock_guard<std::mutex> lock(g_cache.mu);
        auto it = g_cache.free_blocks.find({device, bytes});
        if (it != g_cache.free_blocks.end()) {
            *out = it->second.p;
            g_cache.free_blocks.erase(it);
            g_cache.cached_bytes[device] -= bytes;
            g_cache.live[*out] = {device, bytes};
            return TH_OK;
        }
    }
    hipError_t e = th_malloc_retry(out, bytes);       // (gives the parked blocks back and tries again when the device is full)
    if (e != hipSuccess) {
        (void)hipGetLastError();
        TH_FAIL(e == hipErrorOutOfMemory ? TH_ENOMEM : TH_EHIP, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    }
    std::lock_guard<std::mutex> lock(g_cache.mu);
    g_cache.live[*out] = {device, bytes};
    return TH_OK;
}

void cached_free(void* p) {
    if (!p) return;
    std::vector<void*> evict;
    {
        std::lock_guard<std::mutex> lock(g_cache.mu);
        auto it = g_cache.live.find(p);
        if (it == g_cache.live.end()) { (void)hipFree(p); return; }
        const std::pair<int, size_t> key = it->second;
        g_cache.live.erase(it);
        const size_t cap = cache_cap_locked(key.first);
        if (key.second > cap) evict.push_back(p);               // larger than the whole cache: straight back to HIP
        else {
            // least recently parked blocks of this device make room (round 4 refused the NEW block instead, so a process that
            // loads models of varying size pinned its first 24 GB of stale sizes for ever)
            g_cache.free_blocks.insert({key, {p, ++g_cache.clock}});
            g_cache.cached_bytes[key.first] += key.second;
            while (g_cache.cached_bytes[key.first] > cap || g_cache.free_blocks.size() > DevCache::kCacheBlocks) {
                auto oldest = g_cache.free_blocks.end();
                for (auto b = g_cache.free_blocks.begin(); b != g_cache.free_blocks.end(); ++b)
                    if ((b->first.first == key.first || g_cache.free_blocks.size() > DevCache::kCacheBlocks) &&
                        (oldest == g_cache.free_blocks.end() || b->second.stamp < oldest->second.stamp))
                        oldest = b;
                if (oldest == g_cache.free_blocks.end()) break;
                evict.push_back(oldest->second.p);
                g_cache.cached_bytes[oldest->first.first] -= oldest->first.second;
                g_cache.free_blocks.erase(oldest);
            }
        }
    }
    for (void* q : evict) (void)hipFree(q);
}
}  // namespace

hipError_t th_malloc_retry_impl(void** p, size_t bytes) {
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipErrorOutOfMemory) return e;
    (void)hipGetLastError();
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) return e;
    std::vector<void*> drop;
    {
        std::lock_guard<std::mutex> lock(g_cache.mu);
        for (auto it = g_cache.free_blocks.begin(); it != g_cache.free_blocks.end();) {
            if (it->first.first == device) {
                drop.push_back(it->second.p);
                g_cache.cached_bytes[device] -= it->first.second;
                it = g_cache.free_blocks.erase(it);
            } else ++it;
        }
    }
    if (drop.empty()) return e;
    for (void* q : drop) (void)hipFree(q);
    e = hipMalloc(p, bytes);
    if (e != hipSuccess) (void)hipGetLastError();
    return e;
}

extern "C" int th_dev_trim(int device) {
    std::vector<void*> drop;
    {
        std::lock_guard<std::mutex> lock(g_cache.mu);
        for (auto it = g_cache.free_blocks.begin(); it != g_cache.free_blocks.end();) {
            if (device < 0 || it->first.first == device) {
                drop.push_back(it->second.p);
                g_cache.cached_bytes[it->first.first] -= it->first.second;
                it = g_cache.free_blocks.erase(it);
            } else ++it;
        }
    }
    if (drop.empty()) return TH_OK;                 // nothing cached: no HIP call at all
    for (void* p : drop) (void)hipFree(p);
    return TH_OK;
}

// bytes parked in the block cache of `device` (all devices: -1) and their cap — tests and tools
extern "C" int th_dev_cache_info(int device, uint64_t* cached_bytes, uint64_t* cap_bytes, int* blocks) {
    std::lock_guard<std::mutex> lock(g_cache.mu);
    uint64_t c = 0;
    int n = 0;
    for (auto& kv : g_cache.free_blocks)
        if (device < 0 || kv.first.first == device) { c += kv.first.second; ++n; }
    if (cached_bytes) *cached_bytes = c;
    if (cap_bytes) *cap_bytes = device >= 0 ? cache_cap_locked(device) : DevCache::kCacheBytes;
    if (blocks) *blocks = n;
    return TH_OK;
}

namespace {

// ---- pack (mirrors timed_hip/pack.py) -----------------------------------------------------------
constexpr int kMaxIn = 8, kNIp = 24, kNFp = 8, kNW = 8, kNameBytes = 56;
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

struct Node {
    int op = 0;
    std::vector<int> in;
    int ip[kNIp] = {0};
    float fp[kNFp] = {0};
    int w[kNW] = {-1, -1, -1, -1, -1, -1, -1, -1};
    std::string name;
    int D = 1, H = 1, W = 1, C = 0;  // output shape (rank-1 outputs: D=H=W=1, C=F)
    int rank = 0;
    std::vector<int> consumers;
    // planning state
    int absorbed_by = -1;  // node index of the step that computes this node as part of its chain
    int buf = -1, cs = 0, coff = 0;  // storage of this node's output (if materialised)
    int blk = 0;                     // 4: chunk-blocked storage (TView::blk)
    bool materialised = false;
};

struct Buffer {
    int64_t floats_per_frame = 0;
    float* dev = nullptr;
};

struct Step {
    std::string label;
    std::function<int(hipStream_t, int64_t)> run;
    double flops = 0, exec_flops = 0, bytes = 0;  // per frame
    double direct_flops = -1;     // >= 0: this step's share of the model's direct-form FLOP count when it differs from `flops` (Winograd)
    double ms = 0;
    int64_t launches = 0;
    int out_node = -1;
    bool is_final_softmax = false;
    bool fast = false;            // a minimal-filtering or split-operand form (fast_form): what the load-time guard checks
};

// a remark in a step label, in front of the trailing " [kernel]" that tools/ parse
inline std::string label_note(const std::string& label, const char* note) {
    const size_t k = label.rfind(" [");
    return k == std::string::npos ? label + note : label.substr(0, k) + note + label.substr(k);
}

inline void keras_same_pad(int n, int k, int s, int d, int* before) {
    const int ke = (k - 1) * d + 1;
    const int out = (n + s - 1) / s;
    int total = (out - 1) * s + ke - n;
    if (total < 0) total = 0;
    *before = total / 2;
}

}  // namespace

struct th_model {
    int device = 0;
    int ncu = 0;                  // CUs of `device`: the persistent kernels size their grids by it
    unsigned flags = 0;
    hipStream_t stream = nullptr;
    std::vector<Node> nodes;
    std::vector<const float*> blob_host;  // into `pack`
    std::vector<size_t> blob_count;
    std::vector<char> pack;
    std::vector<float*> dev_allocs;  // weights & derived tensors (freed at th_model_free)
    std::vector<Buffer> bufs;
    std::vector<Step> steps;
    int wino_v_buf = -1, wino_m_buf = -1;   // scratch arenas of the Winograd layers (shared: the layers run one after the other)
    ThKnobs knobs;                          // the TH_* knobs as th_model_load found them (plans and launchers point here)
    // load-time guard (guard_check): 0 not run (TH_GUARD=0, or no fast plan to check), 1 passed, 2 tripped (fast features dropped)
    int guard_state = 0;
    double guard_dlogit = 0, guard_scale = 0;   // max |logit(fast) - logit(direct)| of the plan that is kept, max |logit(direct)|
    double guard_ms = 0;                        // wall time of the check inside th_model_load
    double guard_ref_load_ms = 0, guard_run_ms = 0;
    std::string guard_note;
    int input_node = -1, output_node = -1, logits_node = -1;
    int in_dims[4] = {0, 0, 0, 0};
    int n_classes = 0;
    int chunk = 1024;
    int chunk_alloc = 0;
    int profiling = 0;            // 0 off, 1 every step, 2 only the step with the most algorithmic FLOPs
    int dominant_step = -1;
    std::vector<hipEvent_t> ev_pool;
    double algo_flops = 0, exec_flops = 0;
    // ---- host-buffer pipeline (th_predict / th_predict_async) ----
    // frames travel host -> device in pieces of <= chunk frames through a ring of kRing device buffers on a copy
    // stream; piece g's kernels (model stream) wait for its copy, the copy into a ring slot waits for the kernels
    // that last read it; probabilities return through a pinned host buffer per ticket on a third stream.
    static constexpr int kRing = 3;
    static constexpr int kTickets = 4;
    hipStream_t copy_stream = nullptr, d2h_stream = nullptr;
    void* d_in_ring[kRing] = {nullptr, nullptr, nullptr};
    size_t in_ring_bytes = 0;          // capacity of EACH ring buffer
    void* d_sp_ring[kRing] = {nullptr, nullptr, nullptr};     // sparse transport (th_predict_sparse_async): a piece's bitmaps, ranks
    size_t sp_ring_bytes = 0;                                 // and stored values as they arrive, expanded into d_in_ring[r]
    hipEvent_t ev_h2d[kRing] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_free[kRing] = {nullptr, nullptr, nullptr};
    bool ring_used[kRing] = {false, false, false};
    uint64_t piece_counter = 0;
    // Threading contract (include/timed_hip.h): submissions (th_predict_async / th_predict / th_predict_device) on one
    // handle are serialised by `mu`; th_predict_wait may run on another thread than the submitter.  A ticket slot stays
    // `busy` until its waiter has synchronised on `done` AND copied the rows out, so a concurrent submission can never
    // re-record its events or reallocate its buffers underneath the waiter.
    std::mutex mu;
    struct Ticket {
        bool busy = false;
        bool waiting = false;     // a th_predict_wait call owns this slot right now
        hipEvent_t computed = nullptr, done = nullptr;
        float* d_out = nullptr;  size_t d_out_floats = 0;
        float* h_out = nullptr;  size_t h_out_floats = 0;   // pinned
        float* user_out = nullptr;
        size_t floats = 0;
    } tickets[kTickets];
    int64_t last_n = 0;
    const void* cur_in = nullptr;  // caller's frames for the chunk in flight (first-layer kernel reads them directly)
    int cur_dtype = TH_F32;
    bool need_convert = true;      // some consumer of the input needs the fp32 arena copy

    // ---- two lanes (TH_LANES=2 / th_model_set_lanes): a chunk is cut in two halves that travel through the plan on two
    // streams, the second one a few steps behind the first, each in its own half of every arena.  Layers of different
    // kind then overlap on the device: an HBM-bound 1x1x1 layer (<= 24 KB of LDS, 4-wave workgroups) of one half co-resides
    // with the single 138 KB / 8-wave workgroup per CU of an MFMA-bound 10^3 growth convolution of the other half and runs
    // in its barrier / LDS-write / epilogue gaps, and vice versa.
    int lanes = 1;
    int lane_lag = 1;                 // steps the second lane runs behind the first at issue time
    hipStream_t stream2 = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int64_t lane_off = 0;             // frame offset (inside the arenas) of the lane whose steps are being issued

    TView view(int node) const {
        const Node& nd = nodes[node];
        TView v;
        const Buffer& b = bufs[nd.buf];
        v.p = b.dev + lane_off * b.floats_per_frame;
        v.D = nd.D; v.H = nd.H; v.W = nd.W; v.C = nd.C;
        v.cs = nd.cs; v.coff = nd.coff; v.fs = b.floats_per_frame;
        v.blk = nd.blk;
        return v;
    }
};

namespace {

int upload(th_model* m, const float* h, size_t count, float** out) {
    float* d = nullptr;
    if (int rc = cached_malloc((void**)&d, (count ? count : 1) * sizeof(float), m->device)) return rc;
    m->dev_allocs.push_back(d);
    if (count) HIP_TRY(hipMemcpy(d, h, count * sizeof(float), hipMemcpyHostToDevice));
    *out = d;
    return TH_OK;
}

int parse_pack(th_model* m) {
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
enum class Kern { None, Wino, WfSplit, Wf, First5, First, Pointwise, Gl, Mfma, Direct, DenseGemm, Dense };

// one Conv3D / Dense step: what it absorbs, and the kernel that runs it — decided once, read by every pass after the decision
struct LayerPlan {
    ConvFusion f;
    ConvGeom g{};                 // Conv3D: the geometry on the input it reads (f.src)
    Kern family = Kern::None;     // fusion pass: First5 / First / Pointwise / Mfma with `mp` (None: no MFMA-family plan)
    ConvMfmaPlan mp;
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
           (L.kind == Kern::First && (L.mp.first_wino || L.b3));
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

// the MFMA family of convolution i, in this order: first5 -> first -> pointwise -> mfma.  The fused pool is dropped when the
// kernel that takes the layer cannot pool it.
void choose_family(const Planner& P, int i, LayerPlan& L) {
    ConvFusion& f = L.f;
    const Node& n = P.N[i];
    const Node& src = P.N[f.src];
    const ConvGeom& g = L.g;
    const TView iv = shape_of(src), ov = shape_of(n);
    const int pool = P.pool_mode(f);
    const bool stem = P.use_mfma && P.fuse && f.src == P.m->input_node && f.pre.empty();
    ConvMfmaPlan& mp = L.mp;
    Kern& k = L.family;
    if (stem && pool == 1 && conv_first5_ok(src.D, src.H, src.W, src.C, n.C, g, 1, P.kn)) {
        // ProDCoNN's 5x5x5 stem: direct form on the bf16 pipe, input split once at staging (conv_first5.hip)
        mp = ConvMfmaPlan();
        mp.pool = 1; mp.nnb = 1;
        mp.knobs = &P.kn;
        mp.exec_flops = conv_first5_exec_flops();
        mp.label = conv_first5_label();
        k = Kern::First5;
    }
    if (k == Kern::None && stem && conv_first_plan(src.D, src.H, src.W, src.C, ov, g, n.C, pool, P.kn, &mp)) k = Kern::First;
    if (k == Kern::None && P.use_mfma && g.kd * g.kh * g.kw == 1 && conv_pw_plan(iv, ov, g, src.C, n.C, pool, P.kn, &mp))
        k = Kern::Pointwise;
    if (k == Kern::None && P.use_mfma) {
        if (f.pool >= 0 && conv_mfma_plan(iv, ov, g, src.C, n.C, pool, P.kn, &mp)) k = Kern::Mfma;
        else if (conv_mfma_plan(iv, ov, g, src.C, n.C, 0, P.kn, &mp)) { k = Kern::Mfma; f.pool = -1; }
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
        if (!((pp.family == Kern::Pointwise && pp.mp.pool == 0) || (pp.family == Kern::First && pp.mp.nnb == 1))) continue;
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

// in this order: wino -> wfs -> wf -> first5 -> first -> pointwise -> gl -> mfma -> direct.  After the chunk-blocked pass: the
// wfs and gl kernels read `blk`.
int choose_kernel(Planner& P, int i, LayerPlan& L) {
    th_model* m = P.m;
    if (int rc = build_epilogue(P, i, L)) return rc;
    const Node& n = P.N[i];
    const Node& sn = P.N[L.f.src];
    if (n.op == OP_DENSE) {
        if (sn.cs != sn.C || sn.coff != 0 || sn.D * sn.H * sn.W != 1) TH_FAIL(TH_EUNSUP, "%s: Dense needs a contiguous vector input", n.name.c_str());
        L.kind = P.kn.dense_gemm && dense_gemm_ok(sn.C, n.C, m->bufs[sn.buf].floats_per_frame) ? Kern::DenseGemm : Kern::Dense;
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
             (L.family == Kern::None || L.mp.bres != 3) &&          // (the 16-wide kernel keeps its layers: 42 against 62 us on DenseCPD's 2^3 ones)
             conv_gl_ok(Cin, Cout, sn.cs, sn.coff, (int64_t)m->bufs[sn.buf].floats_per_frame))
        L.kind = Kern::Gl;
    else if (L.family == Kern::Mfma) {
        L.kind = Kern::Mfma;
        // heterogeneous Cout blocks: the last, mostly empty 128-column block on a narrower instantiation
        L.tailed = conv_mfma_plan_tail(iv, ov, g, Cin, Cout, L.mp.pool, L.mp, P.kn, &L.tp, &L.cout_main);
    } else L.kind = Kern::Direct;
    // the aposteriori case (21^3 frames, pool before a monotone chain) runs on the bf16 pipe with split operands
    if (L.kind == Kern::First) L.b3 = conv_first_b3_ok(L.mp, sn.D, sn.H, sn.W, Cin, std::min(Cout, 32), g, L.po);
    L.mp.ncu = L.tp.ncu = L.wfp.ncu = L.sp.ncu = m->ncu;
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
    auto Vp = [M]() { const Buffer& b = M->bufs[M->wino_v_buf]; return b.dev + M->lane_off * b.floats_per_frame; };
    auto Mp = [M]() { const Buffer& b = M->bufs[M->wino_m_buf]; return b.dev + M->lane_off * b.floats_per_frame; };
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

int emit_first5(const ConvArgs& c, const LayerPlan& L, Step& st) {
    float* dw;
    if (int rc = upload_packed(c.M, conv_first5_wpk_floats(), [&](float* d) { conv_first5_pack_weights(c.Cin, c.Cout, c.hw, d); }, &dw))
        return rc;
    st.exec_flops = L.mp.exec_flops;
    st.label = conv_label(c, L.mp.label, false, false);
    const ThKnobs* kn = L.mp.knobs;
    st.run = [=](hipStream_t s, int64_t cnt) {
        return launch_conv_first5(s, cnt, kn, c.M->ncu, c.M->cur_in, c.M->cur_dtype, c.Cin, c.out(), c.Cout, dw, c.bias, c.po);
    };
    return TH_OK;
}

// the first layer on the caller's frames (conv_first.hip, conv_first_b3.hip): one launch per block of 32 output channels, each
// with its own weight columns, bias and per-channel epilogue vectors
int emit_first(const ConvArgs& c, const LayerPlan& L, Step& st) {
    const ConvMfmaPlan mp = L.mp;
    const bool b3 = L.b3;
    if (mp.first_wino) {
        st.direct_flops = st.flops;
        st.flops = mp.own_flops;
    }
    st.exec_flops = b3 ? conv_first_b3_exec_flops() * mp.nnb : mp.exec_flops;
    st.label = conv_label(c, b3 ? conv_first_b3_label(mp.nnb) : conv_first_label(mp, c.Cin, c.po), false, c.node(c.dst).blk);
    if (mp.nnb > 1) st.label = label_note(st.label, (" x" + std::to_string(mp.nnb) + " passes of 32 columns").c_str());
    struct Pass { int c0, cn; float* dw; const float* bias; PostOps po; };
    std::vector<Pass> passes;
    const size_t ktaps = (size_t)c.g.kd * c.g.kh * c.g.kw * c.Cin;
    for (int c0 = 0; c0 < c.Cout; c0 += 32) {
        Pass ps{c0, std::min(32, c.Cout - c0), nullptr, c.bias ? c.bias + c0 : nullptr, post_from(c.po, c0)};
        const std::vector<float> wcol = weight_columns(c.hw, ktaps, c.Cout, c0, ps.cn);
        const int rc = upload_packed(c.M, b3 ? conv_first_b3_wpk_floats() : mp.wpk_floats, [&](float* d) {
            if (b3) conv_first_b3_pack_weights(c.Cin, ps.cn, wcol.data(), d);
            else if (mp.first_wino) conv_first_w_pack_weights(c.Cin, ps.cn, wcol.data(), d);
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
            const int r = b3 ? launch_conv_first_b3(s, cnt, mp, M->cur_in, M->cur_dtype, c.Cin, ov, ps.cn, ps.dw, ps.bias, ps.po)
                             : launch_conv_first(s, cnt, mp, M->cur_in, M->cur_dtype, iD, iH, iW, c.Cin, ov, c.g, ps.cn, ps.dw, ps.bias, ps.po);
            if (r) return r;
        }
        return (int)TH_OK;
    };
    return TH_OK;
}

int emit_pointwise(const ConvArgs& c, const LayerPlan& L, Step& st) {
    const ConvMfmaPlan mp = L.mp;
    float* dw;
    if (int rc = upload_packed(c.M, mp.wpk_floats, [&](float* d) { conv_pw_pack_weights(mp, c.Cin, c.Cout, c.hw, d); }, &dw)) return rc;
    const bool blk = c.node(c.dst).blk != 0;
    st.exec_flops = mp.exec_flops;
    st.label = conv_label(c, conv_pw_label(mp, blk, c.po), false, blk);
    st.run = [=](hipStream_t s, int64_t cnt) { return launch_conv_pw(s, cnt, mp, c.in(), c.out(), c.Cin, c.Cout, dw, c.bias, c.pre, c.po); };
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
    st.label = conv_label(c, mp.label + " x" + std::to_string(mp.nnb) + " + " + tp.label, false, false);
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
        case Kern::First5: rc = emit_first5(c, L, st); break;
        case Kern::First: rc = emit_first(c, L, st); break;
        case Kern::Pointwise: rc = emit_pointwise(c, L, st); break;
        case Kern::Gl: rc = emit_gl(c, st); break;
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
        gp == M->output_node || N[gp].C > 2048)
        return 0;
    const int dn = N[gp].consumers[0];
    if (N[dn].op != OP_DENSE || !P.layers.count(dn) || N[dn].C > 512 || N[dn].w[0] < 0) return 0;
    const ConvFusion& f = P.layers.at(dn).f;
    if (f.src != gp || !f.pre.empty() || !f.post.empty() || f.pool >= 0 || f.last != dn || !N[dn].materialised) return 0;
    // (Dense(activation='softmax') keeps its two steps: logits and probabilities share the node there, and a TH_PREDICT_LOGITS
    // call drops the in-place softmax step)
    if (N[dn].ip[3] != ACT_LINEAR || dn == M->output_node || N[dn].consumers.size() != 1) return 0;
    const int sm = N[dn].consumers[0];                  // node that holds the probabilities
    if (!(N[sm].op == OP_ACT && N[sm].ip[0] == ACT_SOFTMAX && sm == M->output_node && N[sm].absorbed_by < 0 && N[sm].materialised)) return 0;
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

// the load-time planner: the model's graph -> m->steps, a short list of launches
int plan(th_model* m) {
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

int ensure_buffers(th_model* m) {
    if (m->chunk_alloc >= m->chunk) return TH_OK;
    for (Buffer& b : m->bufs) {
        if (b.dev) { cached_free(b.dev); b.dev = nullptr; }
    }
    for (Buffer& b : m->bufs) {
        // (chunk rounded up to 64 frames: the Winograd scratch is addressed in 64-frame GEMM row blocks)
        const size_t bytes = (size_t)b.floats_per_frame * ((m->chunk + 63) / 64 * 64) * sizeof(float) + 256;
        if (int rc = cached_malloc((void**)&b.dev, bytes, m->device)) return rc;
        // channel-padding lanes of the input arena and unused concat lanes must hold finite values
        HIP_TRY(hipMemsetAsync(b.dev, 0, bytes, m->stream));
    }
    m->chunk_alloc = m->chunk;
    return TH_OK;
}

size_t dtype_size(int dt) {
    switch (dt) {
        case TH_F32: return 4;
        case TH_F64: return 8;
        case TH_U8: case TH_BOOL: return 1;
        case TH_F16: return 2;
        default: return 0;
    }
}

int run_device(th_model* m, const void* d_frames, int dtype, int64_t n, float* d_probs, unsigned flags, bool sync = true) {
    const size_t esz = dtype_size(dtype);
    if (!esz) TH_FAIL(TH_EINVAL, "unknown frame dtype %d", dtype);
    if (n < 0) TH_FAIL(TH_EINVAL, "negative frame count");
    HIP_TRY(hipSetDevice(m->device));
    int rc = ensure_buffers(m);
    if (rc) return rc;
    const bool logits = (flags & TH_PREDICT_LOGITS) != 0;
    if (logits && m->logits_node < 0) TH_FAIL(TH_EINVAL, "model does not end in a Softmax: no logits to return");
    const Node& in = m->nodes[m->input_node];
    const int Vin = in.D * in.H * in.W;
    const size_t frame_bytes = (size_t)Vin * in.C * esz;
    const int out_node = logits ? m->logits_node : m->output_node;
    // profiling: events come from a pool owned by the model and consecutive steps share their boundary event
    std::vector<hipEvent_t> evs;      // evs[k], evs[k+1] bracket ev_step[k] when ev_step[k] >= 0
    std::vector<int> ev_step;
    size_t ev_used = 0;
    bool at_event = false;        // the last recorded event marks the current end of the stream
    auto next_event = [&](hipEvent_t* e) -> int {
        if (ev_used == m->ev_pool.size()) {
            hipEvent_t ne;
            HIP_TRY(hipEventCreate(&ne));
            m->ev_pool.push_back(ne);
        }
        *e = m->ev_pool[ev_used++];
        HIP_TRY(hipEventRecord(*e, m->stream));
        return TH_OK;
    };
    for (int64_t off = 0; off < n; off += m->chunk) {
        const int64_t cnt = std::min<int64_t>(m->chunk, n - off);
        m->cur_in = (const char*)d_frames + (size_t)off * frame_bytes;
        m->cur_dtype = dtype;
        if (m->need_convert) {
            rc = launch_convert_frames(m->stream, m->cur_in, dtype, cnt, Vin, in.C, m->view(m->input_node));
            if (rc) return rc;
        }
        const bool two = m->lanes == 2 && !m->profiling && cnt >= 256 && m->stream2;
        if (two) {
            // halves of the chunk on two streams; lane 1 issues `lane_lag` steps behind lane 0
            const int64_t h0 = (cnt / 2 + 63) / 64 * 64, h1 = cnt - h0;
            const char* in0 = (const char*)m->cur_in;
            HIP_TRY(hipEventRecord(m->ev_fork, m->stream));
            HIP_TRY(hipStreamWaitEvent(m->stream2, m->ev_fork, 0));
            std::vector<size_t> order;
            for (size_t si = 0; si < m->steps.size(); ++si)
                if (!(logits && m->steps[si].is_final_softmax)) order.push_back(si);
            const int L = std::max(0, m->lane_lag);
            for (size_t k = 0; k < order.size() + (size_t)L; ++k) {
                if (k < order.size()) {
                    m->lane_off = 0; m->cur_in = in0;
                    if ((rc = m->steps[order[k]].run(m->stream, h0))) { m->lane_off = 0; return rc; }
                }
                if (k >= (size_t)L) {
                    m->lane_off = h0; m->cur_in = in0 + (size_t)h0 * frame_bytes;
                    rc = m->steps[order[k - L]].run(m->stream2, h1);
                    m->lane_off = 0; m->cur_in = in0;
                    if (rc) return rc;
                }
            }
            m->lane_off = 0; m->cur_in = in0;
            HIP_TRY(hipEventRecord(m->ev_join, m->stream2));
            HIP_TRY(hipStreamWaitEvent(m->stream, m->ev_join, 0));
        } else
        for (size_t si = 0; si < m->steps.size(); ++si) {
            Step& st = m->steps[si];
            if (logits && st.is_final_softmax) continue;
            const bool timed = m->profiling == 1 || (m->profiling == 2 && (int)si == m->dominant_step);
            if (timed && !at_event) {   // interval k = (evs[k], evs[k+1]); a fresh start event opens a gap interval
                hipEvent_t e0;
                if ((rc = next_event(&e0))) return rc;
                if (!evs.empty()) ev_step.push_back(-1);
                evs.push_back(e0);
            }
            rc = st.run(m->stream, cnt);
            if (rc) return rc;
            at_event = false;
            if (timed) {
                hipEvent_t e1;
                if ((rc = next_event(&e1))) return rc;
                evs.push_back(e1);
                ev_step.push_back((int)si);
                at_event = true;    // the next step can use e1 as its start
            }
        }
        at_event = false;           // the output copy (and the next chunk's convert) are not steps
        TView o;
        o.p = d_probs + (size_t)off * m->nodes[out_node].C;
        o.C = o.cs = m->nodes[out_node].C;
        o.fs = o.C;
        rc = launch_copy(m->stream, cnt, m->view(out_node), o);
        if (rc) return rc;
        m->last_n = cnt;
    }
    if (!sync && !m->profiling) return TH_OK;  // caller overlaps its next host->device copy and synchronises itself
    HIP_TRY(hipStreamSynchronize(m->stream));
    for (size_t k = 0; k < ev_step.size() && k + 1 < evs.size(); ++k) {
        if (ev_step[k] < 0) continue;
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, evs[k], evs[k + 1]));
        m->steps[ev_step[k]].ms += ms;
        m->steps[ev_step[k]].launches += 1;
    }
    return TH_OK;
}

int load_common(th_model* m, const ThKnobs& knobs) {
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipDeviceGetAttribute(&m->ncu, hipDeviceAttributeMultiprocessorCount, m->device));
    HIP_TRY(hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&m->copy_stream, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&m->d2h_stream, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&m->stream2, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&m->ev_fork, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&m->ev_join, hipEventDisableTiming));
    m->knobs = knobs;       // every A/B / test knob of this handle: the environment as th_model_load_mem read it, or the load-time guard's
    m->lanes = m->knobs.lanes; m->lane_lag = m->knobs.lane_lag;
    for (int r = 0; r < th_model::kRing; ++r) {
        HIP_TRY(hipEventCreateWithFlags(&m->ev_h2d[r], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&m->ev_free[r], hipEventDisableTiming));
    }
    for (th_model::Ticket& t : m->tickets) {
        HIP_TRY(hipEventCreateWithFlags(&t.computed, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&t.done, hipEventDisableTiming));
    }
    int rc = parse_pack(m);
    if (rc) return rc;
    return plan(m);
}


// ---- load-time guard ----------------------------------------------------------------------------------
// The default plan computes most layers in a minimal-filtering form (conv_wino / conv_wfused / k_conv_first_w) and the 5^3 GEMMs
// with bf16x3-split operands.  Their error was measured on the synthetic benchmark weights only; real `.h5` weights have never
// been seen here (reference predict.py:121), and parity is unpinned against TensorFlow.  So every load checks its own plan: a
// second, DIRECT plan of the same pack (fp32-input MFMA kernels only: TH_WINOGRAD=0 TH_WFUSED=0 TH_FIRST_WINO=0) runs a handful
// of internally generated frames, and the logits of the two plans must agree to kGuardTol x max(1, max |logit|).  If they do
// not, fast features are dropped in the order split GEMM -> 5^3 Winograd -> fused 10^3 Winograd -> first-layer F(2,3) until
// they do (the last step IS the direct plan).  th_model_guard_info reports what happened; TH_GUARD=0 switches the check off,
// TH_GUARD_TOL overrides the tolerance (tests force a trip with it).
constexpr int kGuardFrames = 4;
constexpr double kGuardTol = 1e-5;

bool has_fast_steps(const th_model* m) {
    return std::any_of(m->steps.begin(), m->steps.end(), [](const Step& s) { return s.fast; });
}

// deterministic frames of any shape: the first half sparse in [0, 1] (about one voxel-channel in five non-zero, like
// Gaussian-splat frames), the rest with BOTH signs — one dense in [-1, 1], the others sparse in [-4, 4].  (The all-positive
// set alone let a broken operand of the split first layer through — a constant the hardware expanded with the wrong half —
// which only showed on negative inputs: tests/test_gpu_conv_sweep.py caught it, the guard did not.)
void guard_frames(std::vector<float>* out, size_t count) {
    out->assign(count, 0.f);
    uint64_t st = 0x9e3779b97f4a7c15ull;
    const size_t per = std::max<size_t>(1, count / kGuardFrames);
    for (size_t i = 0; i < count; ++i) {
        st = st * 6364136223846793005ull + 1442695040888963407ull;
        const uint32_t r = (uint32_t)(st >> 33);
        const float u = (float)((r >> 8) & 0xffffu) / 65535.f;
        const size_t frame = i / per;
        if (frame < (size_t)kGuardFrames / 2) { if ((r & 15u) < 3u) (*out)[i] = u; }
        else if (frame == (size_t)kGuardFrames / 2) (*out)[i] = 2.f * u - 1.f;
        else if ((r & 15u) < 3u) (*out)[i] = 8.f * u - 4.f;
    }
}

// logits (or the probabilities when the model has no softmax tail) of the guard frames through plan `m`
int guard_run(th_model* m, const float* d_frames, float* d_out, std::vector<float>* h_out) {
    const int keep_chunk = m->chunk;
    m->chunk = 8;
    const unsigned fl = m->logits_node >= 0 ? TH_PREDICT_LOGITS : 0u;
    int rc = run_device(m, d_frames, TH_F32, kGuardFrames, d_out, fl);
    m->chunk = keep_chunk;                       // (chunk_alloc stays 8: the arenas are re-made at the first real predict)
    if (rc) return rc;
    const int C = m->nodes[fl ? m->logits_node : m->output_node].C;
    h_out->resize((size_t)kGuardFrames * C);
    HIP_TRY(hipMemcpy(h_out->data(), d_out, h_out->size() * sizeof(float), hipMemcpyDeviceToHost));
    return TH_OK;
}

// Verdicts of this process: a pack that PASSED under the same knobs on the same device is not measured again (a second load of
// the same model — the bench's legs, a service that reloads — costs the hash of the pack instead of a second plan: ~1 ms instead
// of 20-25).  Only passes are remembered; a trip is re-derived (it has to rebuild the handle anyway).
struct GuardSeen { double dlogit, scale; };
std::mutex g_guard_mu;
std::map<std::string, GuardSeen> g_guard_seen;

std::string guard_key(const th_model* m, double tol) {
    uint64_t h = 1469598103934665603ull;                       // FNV-1a over 8-byte words (+ the tail bytes)
    const std::vector<char>& p = m->pack;
    size_t i = 0;
    for (; i + 8 <= p.size(); i += 8) { uint64_t w; std::memcpy(&w, p.data() + i, 8); h = (h ^ w) * 1099511628211ull; }
    for (; i < p.size(); ++i) h = (h ^ (unsigned char)p[i]) * 1099511628211ull;
    char buf[96];
    snprintf(buf, sizeof buf, "%016llx/%zu/d%d/f%u/t%.3g/", (unsigned long long)h, p.size(), m->device, m->flags, tol);
    return std::string(buf) + m->knobs.nondefault;
}

// Verdicts across processes: predict.py loads one model per call, so a fresh process used to pay the second
// plan every time.  A PASS is also written to a small file — <dir>/guard-<hash>.txt, <dir> = $TH_GUARD_CACHE (a directory; "0" = no
// files), else $XDG_CACHE_HOME/timed_hip, else $HOME/.cache/timed_hip — whose name hashes everything the verdict depends on: the
// pack, knobs, flags, tolerance (guard_key), the device's name and CU count, and THIS build of the library (size + mtime of the
// shared object the code runs from).  The file repeats the full key; a mismatch (hash collision, truncated write) is a miss.
std::string guard_disk_path(const th_model* m, const std::string& key, std::string* full_key) {
    const char* e = getenv("TH_GUARD_CACHE");
    std::string dir;
    if (e && *e) {
        if (!std::strcmp(e, "0")) return "";
        dir = e;
    } else if ((e = getenv("XDG_CACHE_HOME")) && *e) dir = std::string(e) + "/timed_hip";
    else if ((e = getenv("HOME")) && *e) dir = std::string(e) + "/.cache/timed_hip";
    else return "";
    char stamp[160] = "nolib";
    Dl_info info;
    struct stat st;
    if (dladdr((const void*)&th_knobs_read, &info) && info.dli_fname && stat(info.dli_fname, &st) == 0)
        snprintf(stamp, sizeof stamp, "lib%lld.%lld.%ld", (long long)st.st_size, (long long)st.st_mtim.tv_sec, (long)st.st_mtim.tv_nsec);
    hipDeviceProp_t prop;
    std::string dev = "dev?";
    if (hipGetDeviceProperties(&prop, m->device) == hipSuccess) dev = std::string(prop.gcnArchName) + "/" + std::to_string(prop.multiProcessorCount);
    *full_key = key + "|" + stamp + "|" + dev;
    uint64_t h = 1469598103934665603ull;
    for (unsigned char c : *full_key) h = (h ^ c) * 1099511628211ull;
    char name[64];
    snprintf(name, sizeof name, "/guard-%016llx.txt", (unsigned long long)h);
    ::mkdir(dir.substr(0, dir.rfind('/')).c_str(), 0777);      // one missing parent level is created, no more
    ::mkdir(dir.c_str(), 0777);
    return dir + name;
}

bool guard_disk_lookup(const std::string& path, const std::string& full_key, GuardSeen* out) {
    FILE* f = fopen(path.c_str(), "r");
    if (!f) return false;
    char line[1024];
    double d = 0, sc = 0;
    bool ok = fgets(line, sizeof line, f) && sscanf(line, "%la %la", &d, &sc) == 2 && fgets(line, sizeof line, f);
    fclose(f);
    if (!ok) return false;
    size_t n = std::strlen(line);
    while (n && (line[n - 1] == '\n' || line[n - 1] == '\r')) line[--n] = 0;
    if (full_key != line || !(d >= 0) || !(sc >= 0)) return false;
    out->dlogit = d; out->scale = sc;
    return true;
}

void guard_disk_store(const std::string& path, const std::string& full_key, const GuardSeen& v) {
    if (path.empty() || full_key.size() > 900) return;
    char tmp[32];
    snprintf(tmp, sizeof tmp, ".%ld.tmp", (long)getpid());
    const std::string t = path + tmp;
    FILE* f = fopen(t.c_str(), "w");
    if (!f) return;                                             // a read-only home is not an error: the verdict is just not kept
    const bool ok = fprintf(f, "%a %a\n%s\n", v.dlogit, v.scale, full_key.c_str()) > 0;
    if (fclose(f) != 0 || !ok || rename(t.c_str(), path.c_str()) != 0) (void)remove(t.c_str());
}

// *mp is the freshly loaded plan; on return it may have been replaced by a plan with fewer fast features
int guard_check(std::unique_ptr<th_model>* mp, std::function<th_model*(const ThKnobs&, int*)> reload) {
    th_model* m = mp->get();
    if (!m->knobs.guard || !has_fast_steps(m)) return TH_OK;
    double tol = kGuardTol;
    if (const char* e = getenv("TH_GUARD_TOL")) tol = atof(e);        // read at load like every other knob (tests)
    const std::string key = guard_key(m, tol);
    {
        std::lock_guard<std::mutex> lock(g_guard_mu);
        auto it = g_guard_seen.find(key);
        if (it != g_guard_seen.end()) {
            m->guard_state = 1; m->guard_dlogit = it->second.dlogit; m->guard_scale = it->second.scale;
            m->guard_note = "(verdict of an earlier load of this pack in this process)";
            return TH_OK;
        }
    }
    std::string disk_key;
    const std::string disk_path = guard_disk_path(m, key, &disk_key);
    if (!disk_path.empty()) {
        GuardSeen seen;
        if (guard_disk_lookup(disk_path, disk_key, &seen)) {
            m->guard_state = 1; m->guard_dlogit = seen.dlogit; m->guard_scale = seen.scale;
            m->guard_note = "(verdict of an earlier process: " + disk_path + ")";
            std::lock_guard<std::mutex> lock(g_guard_mu);
            if (g_guard_seen.size() < 256) g_guard_seen[key] = seen;
            return TH_OK;
        }
    }
    const Node& in = m->nodes[m->input_node];
    std::vector<float> hf;
    guard_frames(&hf, (size_t)kGuardFrames * in.D * in.H * in.W * in.C);
    float *d_frames = nullptr, *d_out = nullptr;
    int rc;
    if ((rc = cached_malloc((void**)&d_frames, hf.size() * sizeof(float), m->device))) return rc;
    if ((rc = cached_malloc((void**)&d_out, (size_t)kGuardFrames * 4096 * sizeof(float), m->device))) { cached_free(d_frames); return rc; }
    auto done = [&](int code) { cached_free(d_frames); cached_free(d_out); return code; };
    if (m->nodes[m->output_node].C > 4096 || (m->logits_node >= 0 && m->nodes[m->logits_node].C > 4096)) return done(TH_OK);
    {
        const hipError_t e = hipMemcpy(d_frames, hf.data(), hf.size() * sizeof(float), hipMemcpyHostToDevice);
        if (e != hipSuccess) { th_set_error("guard: frame upload failed: %s", hipGetErrorString(e)); return done(TH_EHIP); }
    }
    ThKnobs direct = m->knobs;
    direct.guard = 0; direct.wino_split = 0; direct.first_split = 0; direct.wf_split = 0; direct.winograd = 0; direct.wfused = 0; direct.first_wino = 0;
    int lrc = TH_OK;
    const auto t0 = std::chrono::steady_clock::now();
    std::unique_ptr<th_model, void (*)(th_model*)> ref(reload(direct, &lrc), th_model_free);
    if (!ref) return done(lrc);
    const auto t1 = std::chrono::steady_clock::now();
    m->guard_ref_load_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    std::vector<float> want, got;
    if ((rc = guard_run(ref.get(), d_frames, d_out, &want))) return done(rc);
    m->guard_run_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
    double scale = 0;
    for (float v : want) scale = std::max(scale, (double)std::fabs(v));
    auto diff_of = [&](th_model* x, double* d) -> int {
        int r = guard_run(x, d_frames, d_out, &got);
        if (r) return r;
        double mx = 0;
        for (size_t i = 0; i < got.size(); ++i) {
            const double e = std::fabs((double)got[i] - (double)want[i]);
            mx = std::max(mx, std::isfinite(e) ? e : (std::isfinite(want[i]) ? 1e30 : 0.0));
        }
        *d = mx;
        return TH_OK;
    };
    const double bound = tol * std::max(1.0, scale);
    double d = 0;
    if ((rc = diff_of(m, &d))) return done(rc);
    m->guard_scale = scale;
    if (d <= bound) {
        m->guard_state = 1; m->guard_dlogit = d;
        guard_disk_store(disk_path, disk_key, {d, scale});
        std::lock_guard<std::mutex> lock(g_guard_mu);
        if (g_guard_seen.size() < 256) g_guard_seen[key] = {d, scale};
        return done(TH_OK);
    }
    // tripped: drop fast features one at a time, in the order of how much arithmetic they change
    char note[256];
    std::string hist;
    snprintf(note, sizeof note, "default plan %.3g", d);
    hist = note;
    ThKnobs k = m->knobs;
    k.guard = 0;
    constexpr int kStages = 6;
    const char* names[kStages] = {"TH_WINO_SPLIT=0", "TH_WF_SPLIT=0", "TH_FIRST_SPLIT=0", "TH_WINOGRAD=0", "TH_WFUSED=0", "TH_FIRST_WINO=0"};
    std::string dropped;
    for (int stage = 0; stage < kStages; ++stage) {
        int* field = stage == 0 ? &k.wino_split : stage == 1 ? &k.wf_split : stage == 2 ? &k.first_split : stage == 3 ? &k.winograd : stage == 4 ? &k.wfused : &k.first_wino;
        if (*field == 0) continue;
        *field = 0;
        dropped += (dropped.empty() ? "" : " ");
        dropped += names[stage];
        std::unique_ptr<th_model> alt(reload(k, &lrc));
        if (!alt) return done(lrc);
        double da = 0;
        if ((rc = diff_of(alt.get(), &da))) { th_model_free(alt.release()); return done(rc); }
        snprintf(note, sizeof note, "; %s %.3g", names[stage], da);
        hist += note;
        if (da <= bound || stage == kStages - 1) {
            alt->knobs.guard = m->knobs.guard;
            alt->guard_state = 2; alt->guard_dlogit = da; alt->guard_scale = scale;
            alt->guard_ref_load_ms = m->guard_ref_load_ms; alt->guard_run_ms = m->guard_run_ms;
            snprintf(note, sizeof note, "guard tripped (bound %.3g): ", bound);
            alt->guard_note = std::string(note) + hist + " -> kept with " + dropped;
            alt->knobs.nondefault += (alt->knobs.nondefault.empty() ? "" : " ") + std::string("guard:") + dropped;
            th_model_free(mp->release());
            mp->reset(alt.release());
            return done(TH_OK);
        }
        th_model_free(alt.release());
    }
    // No alternative was accepted: every fast feature was already off in the caller's knobs, so the plan IS the direct plan up to
    // kernels the guard does not switch — and it still differs from the reference plan by more than the bound.  Never report that
    // as a pass: the handle is usable, says "tripped" and carries the measured distance.
    m->guard_state = 2; m->guard_dlogit = d;
    snprintf(note, sizeof note, "guard tripped (bound %.3g): ", bound);
    m->guard_note = std::string(note) + hist + " -> no fast feature left to drop; plan kept as loaded";
    return done(TH_OK);
}

}  // namespace

// =================================== C ABI =======================================================
extern "C" {

int th_version(void) { return 1; }
const char* th_last_error(void) { return g_err; }

int th_device_count(int* n_out) {
    if (!n_out) TH_FAIL(TH_EINVAL, "null argument");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *n_out = 0; TH_FAIL(TH_EHIP, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    *n_out = n;
    return TH_OK;
}

int th_device_info(int device, char* name, size_t name_len, char* arch, size_t arch_len, int* cus) {
    hipDeviceProp_t p;
    HIP_TRY(hipGetDeviceProperties(&p, device));
    if (name && name_len) snprintf(name, name_len, "%s", p.name);
    if (arch && arch_len) snprintf(arch, arch_len, "%s", p.gcnArchName);
    if (cus) *cus = p.multiProcessorCount;
    return TH_OK;
}

int th_model_load_mem(const void* pack, size_t nbytes, int device, unsigned flags, th_model** out) {
    if (!pack || !out) TH_FAIL(TH_EINVAL, "null argument");
    ThKnobs env;            // read here and nowhere else (ThKnobs, common.h), before the device is touched
    int rc = th_knobs_read(&env);
    if (rc) return rc;
    std::unique_ptr<th_model> m(new th_model);
    m->device = device;
    m->flags = flags;
    m->pack.assign((const char*)pack, (const char*)pack + nbytes);
    rc = load_common(m.get(), env);
    if (rc) { th_model_free(m.release()); return rc; }
    auto reload = [&](const ThKnobs& k, int* lrc) -> th_model* {          // another plan of the same pack under other knobs
        std::unique_ptr<th_model> x(new th_model);
        x->device = device;
        x->flags = flags;
        x->pack.assign((const char*)pack, (const char*)pack + nbytes);
        *lrc = load_common(x.get(), k);
        if (*lrc) { th_model_free(x.release()); return nullptr; }
        return x.release();
    };
    const auto g0 = std::chrono::steady_clock::now();
    rc = guard_check(&m, reload);
    if (rc) { th_model_free(m.release()); return rc; }
    m->guard_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - g0).count();
    *out = m.release();
    return TH_OK;
}

int th_model_load(const char* pack_path, int device, unsigned flags, th_model** out) {
    if (!pack_path || !out) TH_FAIL(TH_EINVAL, "null argument");
    FILE* f = fopen(pack_path, "rb");
    if (!f) TH_FAIL(TH_EIO, "cannot open %s", pack_path);
    fseek(f, 0, SEEK_END);
    long sz = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<char> buf(sz > 0 ? (size_t)sz : 0);
    const size_t got = sz > 0 ? fread(buf.data(), 1, (size_t)sz, f) : 0;
    fclose(f);
    if ((long)got != sz) TH_FAIL(TH_EIO, "short read on %s", pack_path);
    return th_model_load_mem(buf.data(), buf.size(), device, flags, out);
}

void th_model_free(th_model* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    // queued kernels and copies may still read the arenas: drain the three streams before anything is released
    if (m->stream) (void)hipStreamSynchronize(m->stream);
    if (m->copy_stream) (void)hipStreamSynchronize(m->copy_stream);
    if (m->d2h_stream) (void)hipStreamSynchronize(m->d2h_stream);
    if (m->stream2) (void)hipStreamSynchronize(m->stream2);
    for (float* p : m->dev_allocs) cached_free(p);
    for (Buffer& b : m->bufs) if (b.dev) cached_free(b.dev);
    for (int r = 0; r < th_model::kRing; ++r) {
        if (m->d_in_ring[r]) cached_free(m->d_in_ring[r]);
        if (m->d_sp_ring[r]) cached_free(m->d_sp_ring[r]);
        if (m->ev_h2d[r]) (void)hipEventDestroy(m->ev_h2d[r]);
        if (m->ev_free[r]) (void)hipEventDestroy(m->ev_free[r]);
    }
    for (th_model::Ticket& t : m->tickets) {
        if (t.d_out) cached_free(t.d_out);
        if (t.h_out) (void)hipHostFree(t.h_out);
        if (t.computed) (void)hipEventDestroy(t.computed);
        if (t.done) (void)hipEventDestroy(t.done);
    }
    if (m->stream2) (void)hipStreamDestroy(m->stream2);
    if (m->ev_fork) (void)hipEventDestroy(m->ev_fork);
    if (m->ev_join) (void)hipEventDestroy(m->ev_join);
    if (m->copy_stream) (void)hipStreamDestroy(m->copy_stream);
    if (m->d2h_stream) (void)hipStreamDestroy(m->d2h_stream);
    for (hipEvent_t e : m->ev_pool) (void)hipEventDestroy(e);
    if (m->stream) (void)hipStreamDestroy(m->stream);
    delete m;
}

int th_model_info(const th_model* m, int dims[4], int* n_classes) {
    if (!m) TH_FAIL(TH_EINVAL, "null model");
    if (dims) std::memcpy(dims, m->in_dims, sizeof m->in_dims);
    if (n_classes) *n_classes = m->n_classes;
    return TH_OK;
}

int th_model_cost(const th_model* m, double* algo_flops, double* exec_flops, int* n_steps) {
    if (!m) TH_FAIL(TH_EINVAL, "null model");
    if (algo_flops) *algo_flops = m->algo_flops;
    if (exec_flops) *exec_flops = m->exec_flops;
    if (n_steps) *n_steps = (int)m->steps.size();
    return TH_OK;
}

int th_model_set_chunk(th_model* m, int frames_per_chunk) {
    if (!m || frames_per_chunk <= 0) TH_FAIL(TH_EINVAL, "bad chunk size");
    m->chunk = frames_per_chunk;
    return TH_OK;
}

int th_predict_device(th_model* m, const void* d_frames, int dtype, int64_t n, float* d_probs, unsigned flags) {
    if (n < 0) TH_FAIL(TH_EINVAL, "negative frame count");
    if (!m || (n > 0 && (!d_frames || !d_probs))) TH_FAIL(TH_EINVAL, "null argument");
    std::lock_guard<std::mutex> lock(m->mu);
    return run_device(m, d_frames, dtype, n, d_probs, flags);
}

// Is `p` page-locked host memory the runtime knows (th_host_alloc / th_host_register / hipHostMalloc)?  Copies from
// such memory are truly asynchronous; anything else is pageable and the copy call itself blocks the host.
static bool host_ptr_is_pinned(const void* p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}

// a batch of sparse float32 frames in HOST memory (the sections of a THSPF001 blob, include/timed_hip.h)
struct SparseBatch {
    const uint64_t* vidx;      // [n + 1] cumulative stored-element counts
    const uint32_t* bits;      // [n][W]
    const float* values;       // values[vidx[i] - vidx[0] ...] belong to frame i
    int E, W;
};
static int predict_async_locked(th_model* m, const void* frames, int dtype, int64_t n, float* probs_out, unsigned flags, int* ticket,
                                const SparseBatch* sp = nullptr);

int th_predict_async(th_model* m, const void* frames, int dtype, int64_t n, float* probs_out, unsigned flags, int* ticket) {
    if (n < 0) TH_FAIL(TH_EINVAL, "negative frame count");
    if (!m || !ticket || (n > 0 && (!frames || !probs_out))) TH_FAIL(TH_EINVAL, "null argument");
    std::lock_guard<std::mutex> lock(m->mu);
    int rc = predict_async_locked(m, frames, dtype, n, probs_out, flags, ticket);
    if (rc) {
        // part of the batch may already be queued: nothing of it may still read the caller's frames (or write a ticket
        // buffer the next submission reallocates) once the error has been returned
        const std::string keep = th_last_error();
        (void)hipStreamSynchronize(m->copy_stream);
        (void)hipStreamSynchronize(m->stream);
        (void)hipStreamSynchronize(m->d2h_stream);
        (void)hipGetLastError();
        th_set_error("%s", keep.c_str());
    }
    return rc;
}

static int predict_async_locked(th_model* m, const void* frames, int dtype, int64_t n, float* probs_out, unsigned flags, int* ticket,
                                const SparseBatch* sp) {
    const size_t esz = dtype_size(dtype);
    if (!esz) TH_FAIL(TH_EINVAL, "unknown frame dtype %d", dtype);
    HIP_TRY(hipSetDevice(m->device));
    const Node& in = m->nodes[m->input_node];
    const size_t frame_bytes = (size_t)in.D * in.H * in.W * in.C * esz;
    const bool logits = (flags & TH_PREDICT_LOGITS) != 0;
    if (logits && m->logits_node < 0) TH_FAIL(TH_EINVAL, "model does not end in a Softmax: no logits to return");
    const int width = logits ? m->nodes[m->logits_node].C : m->n_classes;
    int ti = -1;
    for (int k = 0; k < th_model::kTickets; ++k) if (!m->tickets[k].busy) { ti = k; break; }
    if (ti < 0) TH_FAIL(TH_EBUSY, "all %d tickets of this model are in flight: call th_predict_wait first", th_model::kTickets);
    th_model::Ticket& t = m->tickets[ti];
    // A batch that fits one chunk is NOT cut further: measured, 125-frame pieces under-fill the 256 CUs and lose
    // more than the overlap wins.  Overlap across small batches comes from submitting the next ticket early.
    const int64_t piece = std::min<int64_t>(m->chunk, std::max<int64_t>(n, 1));
    const size_t need_in = frame_bytes * (size_t)piece;
    if (!(flags & TH_PREDICT_IN_DEVICE) && m->in_ring_bytes < need_in) {
        // growing the ring: nothing may still be reading the old buffers
        HIP_TRY(hipStreamSynchronize(m->copy_stream));
        HIP_TRY(hipStreamSynchronize(m->stream));
        for (int r = 0; r < th_model::kRing; ++r) {
            if (m->d_in_ring[r]) cached_free(m->d_in_ring[r]);
            m->d_in_ring[r] = nullptr;
            m->ring_used[r] = false;
        }
        m->in_ring_bytes = 0;
        for (int r = 0; r < th_model::kRing; ++r)
            if (int rc = cached_malloc(&m->d_in_ring[r], need_in, m->device)) return rc;
        m->in_ring_bytes = need_in;
    }
    const size_t floats = (size_t)n * width;
    const bool out_on_device = (flags & TH_PREDICT_OUT_DEVICE) != 0;   // probs_out is device memory: no copy back
    if (!out_on_device && t.d_out_floats < floats) {
        if (t.d_out) cached_free(t.d_out);
        t.d_out = nullptr; t.d_out_floats = 0;
        if (int rc = cached_malloc((void**)&t.d_out, std::max<size_t>(floats, 1024) * sizeof(float), m->device)) return rc;
        t.d_out_floats = std::max<size_t>(floats, 1024);
    }
    if (!out_on_device && t.h_out_floats < floats) {
        if (t.h_out) HIP_TRY(hipHostFree(t.h_out));
        t.h_out = nullptr; t.h_out_floats = 0;
        HIP_TRY(hipHostMalloc((void**)&t.h_out, std::max<size_t>(floats, 1024) * sizeof(float), hipHostMallocDefault));
        t.h_out_floats = std::max<size_t>(floats, 1024);
    }
    const bool in_device = (flags & TH_PREDICT_IN_DEVICE) != 0;         // frames are on the device already: no ring, no copies
    const bool pinned = !in_device && n > 0 && host_ptr_is_pinned(sp ? (const void*)sp->values : frames);
    // (Shorter first pieces do not help: PCIe moves 252 k fp32 frames/s against 216 k computed, so a copy only stays
    // hidden behind the previous piece's kernels if pieces grow by <= 1.17x — measured, a 256/512/1024 ramp ends within
    // 0.5 % of equal pieces.  The one unhidden copy costs ~4 ms per call: 0.94x the device-resident rate at 16 k frames,
    // 0.97x at 32 k.)
    if (in_device && n > 0) {
        int rc = run_device(m, frames, dtype, n, (out_on_device ? probs_out : t.d_out), flags, /*sync=*/false);
        if (rc) return rc;
    }
    for (int64_t off = 0; off < n && !in_device; off += piece) {
        const int64_t cnt = std::min<int64_t>(piece, n - off);
        const int r = (int)(m->piece_counter % th_model::kRing);
        if (m->ring_used[r]) {
            // the kernels of the piece that used this ring buffer three pieces ago must have finished with it
            if (pinned) HIP_TRY(hipStreamWaitEvent(m->copy_stream, m->ev_free[r], 0));
            else HIP_TRY(hipEventSynchronize(m->ev_free[r]));
        }
        if (sp) {
            // sparse transport: the piece's bitmaps, ranks and stored values travel (a tenth of the dense bytes for Gaussian frames);
            // k_sparse_expand rebuilds the dense frames in the ring buffer, on the compute stream, in front of the first layer
            const size_t bits_b = (size_t)cnt * sp->W * 4, vidx_b = (size_t)(cnt + 1) * 8;
            const uint64_t v0 = sp->vidx[off], v1 = sp->vidx[off + cnt];
            const size_t val_b = (size_t)(v1 - v0) * 4;
            const size_t o_vidx = (bits_b + 15) / 16 * 16, o_val = (o_vidx + vidx_b + 15) / 16 * 16, need = o_val + val_b + 16;
            if (m->sp_ring_bytes < need) {
                HIP_TRY(hipStreamSynchronize(m->copy_stream));
                HIP_TRY(hipStreamSynchronize(m->stream));
                for (int q = 0; q < th_model::kRing; ++q) {
                    if (m->d_sp_ring[q]) cached_free(m->d_sp_ring[q]);
                    m->d_sp_ring[q] = nullptr;
                }
                m->sp_ring_bytes = 0;
                const size_t cap = need + need / 4;
                for (int q = 0; q < th_model::kRing; ++q)
                    if (int rc = cached_malloc(&m->d_sp_ring[q], cap, m->device)) return rc;
                m->sp_ring_bytes = cap;
            }
            char* const d = (char*)m->d_sp_ring[r];
            HIP_TRY(hipMemcpyAsync(d, sp->bits + (size_t)off * sp->W, bits_b, hipMemcpyHostToDevice, m->copy_stream));
            HIP_TRY(hipMemcpyAsync(d + o_vidx, sp->vidx + off, vidx_b, hipMemcpyHostToDevice, m->copy_stream));
            if (val_b) HIP_TRY(hipMemcpyAsync(d + o_val, sp->values + (v0 - sp->vidx[0]), val_b, hipMemcpyHostToDevice, m->copy_stream));
            HIP_TRY(hipEventRecord(m->ev_h2d[r], m->copy_stream));
            HIP_TRY(hipStreamWaitEvent(m->stream, m->ev_h2d[r], 0));
            int rc = launch_sparse_expand(m->stream, cnt, (const uint32_t*)d, (const uint64_t*)(d + o_vidx), (const float*)(d + o_val),
                                          (float*)m->d_in_ring[r], sp->E, sp->W);
            if (rc) return rc;
        } else {
        HIP_TRY(hipMemcpyAsync(m->d_in_ring[r], (const char*)frames + (size_t)off * frame_bytes, (size_t)cnt * frame_bytes,
                               hipMemcpyHostToDevice, m->copy_stream));
        HIP_TRY(hipEventRecord(m->ev_h2d[r], m->copy_stream));
        HIP_TRY(hipStreamWaitEvent(m->stream, m->ev_h2d[r], 0));
        }
        int rc = run_device(m, m->d_in_ring[r], dtype, cnt, (out_on_device ? probs_out : t.d_out) + (size_t)off * width, flags,
                            /*sync=*/false);
        if (rc) return rc;
        HIP_TRY(hipEventRecord(m->ev_free[r], m->stream));
        m->ring_used[r] = true;
        m->piece_counter++;
    }
    HIP_TRY(hipEventRecord(t.computed, m->stream));
    HIP_TRY(hipStreamWaitEvent(m->d2h_stream, t.computed, 0));
    if (floats && !out_on_device)
        HIP_TRY(hipMemcpyAsync(t.h_out, t.d_out, floats * sizeof(float), hipMemcpyDeviceToHost, m->d2h_stream));
    HIP_TRY(hipEventRecord(t.done, m->d2h_stream));
    t.user_out = probs_out;
    t.floats = out_on_device ? 0 : floats;
    t.busy = true;
    *ticket = ti;
    return TH_OK;
}

// ---- a sparse batch is checked completely on the host before any of it is queued: k_sparse_expand trusts its bitmaps ----
// stored elements of one frame: the set bits of its W bitmap words (W is a multiple of 4 and a frame's words are 16-byte aligned
// in the blob, so they are read as W / 2 64-bit words).  The library is built for baseline x86-64, whose popcount is a dozen
// shift-and-mask operations per word: the POPCNT instruction comes in through a function-level target and a check of the CPU.
static uint64_t popcount_words_portable(const uint64_t* p, size_t n) {
    uint64_t c = 0;
    for (size_t i = 0; i < n; ++i) c += (uint64_t)__builtin_popcountll(p[i]);
    return c;
}
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
__attribute__((target("popcnt"))) static uint64_t popcount_words_hw(const uint64_t* p, size_t n) {
    uint64_t c0 = 0, c1 = 0;
    size_t i = 0;
    for (; i + 2 <= n; i += 2) { c0 += (uint64_t)__builtin_popcountll(p[i]); c1 += (uint64_t)__builtin_popcountll(p[i + 1]); }
    if (i < n) c0 += (uint64_t)__builtin_popcountll(p[i]);
    return c0 + c1;
}
static uint64_t popcount_words(const uint64_t* p, size_t n) {
    static const bool hw = __builtin_cpu_supports("popcnt");
    return hw ? popcount_words_hw(p, n) : popcount_words_portable(p, n);
}
#else
static uint64_t popcount_words(const uint64_t* p, size_t n) { return popcount_words_portable(p, n); }
#endif

// every frame's bitmap against its rank delta, and no bit at or beyond element E (the tail of the last real word, the padding
// words): a bitmap with more bits than the frame has values makes the kernel read past the values that travelled with the piece
static int check_sparse_bitmaps(const SparseBatch& sp, uint32_t n) {
    const uint32_t E = (uint32_t)sp.E, W = (uint32_t)sp.W, full = E / 32, tail = E % 32;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t* const b = sp.bits + (size_t)i * W;
        const uint64_t stored = popcount_words((const uint64_t*)b, W / 2), want = sp.vidx[i + 1] - sp.vidx[i];
        uint32_t beyond = tail ? b[full] >> tail : 0;
        for (uint32_t w = full + (tail ? 1 : 0); w < W; ++w) beyond |= b[w];
        if (beyond) TH_FAIL(TH_EINVAL, "sparse batch: frame %u has bits set beyond its %u elements", i, E);
        if (stored != want)
            TH_FAIL(TH_EINVAL, "sparse batch: frame %u has %llu bits set, its ranks say %llu stored elements", i, (unsigned long long)stored,
                    (unsigned long long)want);
    }
    return TH_OK;
}

int th_predict_sparse_async(th_model* m, const void* blob, size_t blob_bytes, float* probs_out, unsigned flags, int* ticket) {
    if (!m || !ticket || !blob) TH_FAIL(TH_EINVAL, "null argument");
    if (flags & TH_PREDICT_IN_DEVICE) TH_FAIL(TH_EINVAL, "a sparse batch is host memory");
    const char* const b = (const char*)blob;
    if ((uintptr_t)blob % 16) TH_FAIL(TH_EINVAL, "sparse batch: the blob is not 16-byte aligned");
    if (blob_bytes < 32 || std::memcmp(b, TH_SPARSE_MAGIC, 8)) TH_FAIL(TH_EINVAL, "not a THSPF001 sparse frame batch");
    uint32_t n32, E, W, esz;
    uint64_t nval;
    std::memcpy(&n32, b + 8, 4); std::memcpy(&E, b + 12, 4); std::memcpy(&W, b + 16, 4); std::memcpy(&esz, b + 20, 4); std::memcpy(&nval, b + 24, 8);
    const Node& in = m->nodes[m->input_node];
    if (esz != 4 || (int64_t)E != (int64_t)in.D * in.H * in.W * in.C)
        TH_FAIL(TH_EINVAL, "sparse batch: %u elements of %u bytes per frame, the model reads %d float32", E, esz, in.D * in.H * in.W * in.C);
    if (W < (E + 31) / 32 || W % 4) TH_FAIL(TH_EINVAL, "sparse batch: %u bitmap words per frame for %u elements", W, E);
    if (W > (uint32_t)kSpMaxWords)
        TH_FAIL(TH_EINVAL, "sparse batch: %u bitmap words per frame, frames travel sparse with at most %d words (%d elements)", W, kSpMaxWords,
                kSpMaxWords * 32);
    // (n32 < 2^32 and W <= 4096: the offsets cannot wrap; the value count is bounded by a division, not by a sum that can)
    const size_t o_vidx = 32, o_bits = (o_vidx + ((size_t)n32 + 1) * 8 + 15) / 16 * 16, o_val = o_bits + (size_t)n32 * W * 4;
    if (blob_bytes < o_val || nval > (blob_bytes - o_val) / 4)
        TH_FAIL(TH_EINVAL, "sparse batch: %zu bytes, its header describes %u frames and %llu values", blob_bytes, n32, (unsigned long long)nval);
    SparseBatch sp;
    sp.vidx = (const uint64_t*)(b + o_vidx); sp.bits = (const uint32_t*)(b + o_bits); sp.values = (const float*)(b + o_val);
    sp.E = (int)E; sp.W = (int)W;
    if (n32 && (sp.vidx[n32] - sp.vidx[0] != nval)) TH_FAIL(TH_EINVAL, "sparse batch: the ranks end at %llu, the header says %llu values",
                                                                   (unsigned long long)(sp.vidx[n32] - sp.vidx[0]), (unsigned long long)nval);
    for (uint32_t i = 0; i < n32; ++i)
        if (sp.vidx[i + 1] < sp.vidx[i] || sp.vidx[i + 1] - sp.vidx[i] > E) TH_FAIL(TH_EINVAL, "sparse batch: frame %u has an impossible stored-element count", i);
    if (int rc = check_sparse_bitmaps(sp, n32)) return rc;
    if (n32 > 0 && !probs_out) TH_FAIL(TH_EINVAL, "null argument");
    std::lock_guard<std::mutex> lock(m->mu);
    int rc = predict_async_locked(m, blob, TH_F32, n32, probs_out, flags, ticket, &sp);
    if (rc) {
        const std::string keep = th_last_error();
        (void)hipStreamSynchronize(m->copy_stream);
        (void)hipStreamSynchronize(m->stream);
        (void)hipStreamSynchronize(m->d2h_stream);
        (void)hipGetLastError();
        th_set_error("%s", keep.c_str());
    }
    return rc;
}

int th_predict_wait(th_model* m, int ticket) {
    if (!m || ticket < 0 || ticket >= th_model::kTickets) TH_FAIL(TH_EINVAL, "bad ticket");
    th_model::Ticket& t = m->tickets[ticket];
    {
        std::lock_guard<std::mutex> lock(m->mu);
        if (!t.busy) TH_FAIL(TH_EINVAL, "ticket %d is not in flight", ticket);
        if (t.waiting) TH_FAIL(TH_EBUSY, "ticket %d is already being waited on by another thread", ticket);
        t.waiting = true;
    }
    // the blocking part runs WITHOUT the model lock (the submitter keeps queueing the next batches meanwhile); the slot
    // stays busy, so nothing can re-record t.done or touch t.h_out / t.user_out until the rows have been copied out
    int rc = TH_OK;
    hipError_t e = hipSetDevice(m->device);
    if (e == hipSuccess) e = hipEventSynchronize(t.done);
    if (e != hipSuccess) {
        th_set_error("th_predict_wait: %s", hipGetErrorString(e));
        rc = TH_EHIP;
    } else if (t.floats) {
        std::memcpy(t.user_out, t.h_out, t.floats * sizeof(float));
    }
    std::lock_guard<std::mutex> lock(m->mu);
    t.waiting = false;
    t.busy = false;      // success or failure, the slot is returned — but only now
    return rc;
}

int th_predict(th_model* m, const void* frames, int dtype, int64_t n, float* probs_out, unsigned flags) {
    int ticket = -1;
    int rc = th_predict_async(m, frames, dtype, n, probs_out, flags, &ticket);
    if (rc) return rc;
    return th_predict_wait(m, ticket);
}

// ---- page-locked host memory --------------------------------------------------------------------
int th_host_alloc(size_t bytes, void** out) {
    if (!out) TH_FAIL(TH_EINVAL, "null argument");
    HIP_TRY(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
    return TH_OK;
}
int th_host_free(void* p) {
    if (p) HIP_TRY(hipHostFree(p));
    return TH_OK;
}
int th_host_register(void* p, size_t bytes) {
    if (!p || !bytes) TH_FAIL(TH_EINVAL, "null argument");
    HIP_TRY(hipHostRegister(p, bytes, hipHostRegisterDefault));
    return TH_OK;
}
int th_host_unregister(void* p) {
    if (!p) TH_FAIL(TH_EINVAL, "null argument");
    HIP_TRY(hipHostUnregister(p));
    return TH_OK;
}

int th_model_fetch(th_model* m, const char* layer_name, int64_t n, float* out, int64_t out_floats) {
    if (!m || !layer_name || !out) TH_FAIL(TH_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(m->device));
    for (size_t i = 0; i < m->nodes.size(); ++i) {
        const Node& nd = m->nodes[i];
        if (nd.name != layer_name) continue;
        if (!nd.materialised || nd.buf < 0 || nd.blk) TH_FAIL(TH_EINVAL, "layer %s is fused away (load with TH_LOAD_KEEP_ALL)", layer_name);
        if (n > m->last_n) TH_FAIL(TH_EINVAL, "only %lld frames in the last chunk", (long long)m->last_n);
        const int64_t per = (int64_t)nd.D * nd.H * nd.W * nd.C;
        if (out_floats < n * per) TH_FAIL(TH_EINVAL, "output buffer too small (%lld < %lld)", (long long)out_floats, (long long)(n * per));
        float* d = nullptr;
        HIP_TRY(th_malloc_retry((void**)&d, (size_t)(n * per) * sizeof(float) + 16));
        TView o;
        o.p = d; o.D = nd.D; o.H = nd.H; o.W = nd.W; o.C = o.cs = nd.C; o.fs = per;
        int rc = launch_copy(m->stream, n, m->view((int)i), o);
        if (!rc) {
            hipError_t e = hipStreamSynchronize(m->stream);
            if (e == hipSuccess) e = hipMemcpy(out, d, (size_t)(n * per) * sizeof(float), hipMemcpyDeviceToHost);
            if (e != hipSuccess) { th_set_error("fetch copy failed: %s", hipGetErrorString(e)); rc = TH_EHIP; }
        }
        (void)hipFree(d);
        return rc;
    }
    TH_FAIL(TH_EINVAL, "no layer named %s", layer_name);
}

int th_model_profile(th_model* m, int enable) {
    if (!m) TH_FAIL(TH_EINVAL, "null model");
    if (enable < 0 || enable > 2) TH_FAIL(TH_EINVAL, "profile mode must be 0, 1 or 2");
    m->profiling = enable;
    // mode 2 brackets the DOMINANT step only: the one that took the most device time in a preceding mode-1 run (bench.py's
    // warm-up), else the one with the most FLOPs
    m->dominant_step = -1;
    double best = -1;
    bool timed = false;
    for (const Step& s : m->steps) timed = timed || s.launches > 0;
    for (size_t i = 0; i < m->steps.size(); ++i) {
        const double v = timed ? m->steps[i].ms : m->steps[i].flops;
        if (v > best) { best = v; m->dominant_step = (int)i; }
    }
    for (Step& s : m->steps) { s.ms = 0; s.launches = 0; }
    return TH_OK;
}

int th_model_step_info(const th_model* m, int i, char* label, size_t label_len, double* ms, int64_t* launches,
                       double* flops_per_frame, double* exec_flops_per_frame, double* bytes_per_frame) {
    if (!m || i < 0 || i >= (int)m->steps.size()) TH_FAIL(TH_EINVAL, "bad step index");
    const Step& s = m->steps[i];
    if (label && label_len) snprintf(label, label_len, "%s", s.label.c_str());
    if (ms) *ms = s.ms;
    if (launches) *launches = s.launches;
    if (flops_per_frame) *flops_per_frame = s.flops;
    if (exec_flops_per_frame) *exec_flops_per_frame = s.exec_flops;
    if (bytes_per_frame) *bytes_per_frame = s.bytes;
    return TH_OK;
}

int th_model_step_direct_flops(const th_model* m, int i, double* direct_flops_per_frame) {
    if (!m || i < 0 || i >= (int)m->steps.size() || !direct_flops_per_frame) TH_FAIL(TH_EINVAL, "bad step index");
    *direct_flops_per_frame = m->steps[i].direct_flops;
    return TH_OK;
}

int th_model_guard_info(const th_model* m, int* state, double* max_dlogit, double* logit_scale, char* note, size_t note_len) {
    if (!m) TH_FAIL(TH_EINVAL, "null model");
    if (state) *state = m->guard_state;
    if (max_dlogit) *max_dlogit = m->guard_dlogit;
    if (logit_scale) *logit_scale = m->guard_scale;
    if (note && note_len) {
        if (m->guard_state == 0) snprintf(note, note_len, "%s", m->guard_note.c_str());
        else snprintf(note, note_len, "%s%s[%.1f ms: direct plan load %.1f, its run %.1f]", m->guard_note.c_str(), m->guard_note.empty() ? "" : " ",
                      m->guard_ms, m->guard_ref_load_ms, m->guard_run_ms);
    }
    return TH_OK;
}

int th_model_knobs(const th_model* m, char* buf, size_t buf_len) {
    if (!m || !buf || !buf_len) TH_FAIL(TH_EINVAL, "null argument");
    snprintf(buf, buf_len, "%s", m->knobs.nondefault.c_str());
    return TH_OK;
}

// ---- device memory helpers ---------------------------------------------------------------------
int th_dev_alloc(int device, size_t bytes, void** d_out) {
    if (!d_out) TH_FAIL(TH_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(th_malloc_retry(d_out, bytes ? bytes : 1));
    return TH_OK;
}
int th_dev_free(int device, void* d) {
    HIP_TRY(hipSetDevice(device));
    if (d) HIP_TRY(hipFree(d));
    return TH_OK;
}
int th_dev_upload(int device, void* d_dst, const void* h_src, size_t bytes) {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMemcpy(d_dst, h_src, bytes, hipMemcpyHostToDevice));
    return TH_OK;
}
int th_dev_download(int device, void* h_dst, const void* d_src, size_t bytes) {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMemcpy(h_dst, d_src, bytes, hipMemcpyDeviceToHost));
    return TH_OK;
}
int th_dev_sync(int device) {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipDeviceSynchronize());
    return TH_OK;
}
int th_dev_synth_frames(int device, float* d_frames, int64_t n, int side, int channels, int atoms, uint64_t seed) {
    if (!d_frames || n < 0 || side <= 0 || channels <= 0 || atoms < 0) TH_FAIL(TH_EINVAL, "bad argument");
    HIP_TRY(hipSetDevice(device));
    int rc = launch_synth_frames(nullptr, d_frames, n, side, channels, atoms, seed);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    return TH_OK;
}

// ---- sampler -----------------------------------------------------------------------------------
int th_apply_temp(const double* probs, int64_t n_res, int n_cls, double t, double* out) {
    if (!out) TH_FAIL(TH_EINVAL, "null argument");
    return sampler_run(0, probs, n_res, n_cls, 0, t, TH_RNG_PHILOX, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, out);
}
int th_apply_temp_on(int device, const double* probs, int64_t n_res, int n_cls, double t, double* out) {
    if (!out) TH_FAIL(TH_EINVAL, "null argument");
    return sampler_run(device, probs, n_res, n_cls, 0, t, TH_RNG_PHILOX, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, out);
}
int th_sample(const double* probs, int64_t n_res, int n_cls, int64_t n_samples, double temperature, int rng_mode,
              uint64_t seed, const double* uniforms, int32_t* idx_out) {
    if (!idx_out) TH_FAIL(TH_EINVAL, "null argument");
    return sampler_run(0, probs, n_res, n_cls, n_samples, temperature, rng_mode, seed, 0, uniforms, idx_out, nullptr,
                       nullptr, nullptr, nullptr);
}
int th_sample_ex(const double* probs, int64_t n_res, int n_cls, int64_t n_samples, double temperature, int rng_mode,
                 uint64_t seed, uint64_t rng_offset, const double* uniforms, int32_t* idx_out, double* r_out,
                 const char* cat_letters, char* letters_out, double* q_out, int device) {
    return sampler_run(device, probs, n_res, n_cls, n_samples, temperature, rng_mode, seed, rng_offset, uniforms, idx_out,
                       r_out, cat_letters, letters_out, q_out);
}

}  // extern "C"
