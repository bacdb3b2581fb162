// Model runtime, internal: the handle behind include/timed_hip.h's th_model and the functions of one unit that another calls.
//   devcache.hip  per-process device block cache          planner.hip  pack parser, layer-graph planner (parse_pack, plan)
//   guard.hip     load-time guard (guard_check)            predict.hip  executor, host-buffer pipeline, the th_predict* ABI
//   runtime.hip   errors, TH_* knobs, load_common, ~th_model and the rest of the C ABI
#pragma once
#include "common.h"

#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

namespace th_rt {

// ---- pack (mirrors timed_hip/pack.py) -----------------------------------------------------------
constexpr int kMaxIn = 8, kNIp = 24, kNFp = 8, kNW = 8, kNameBytes = 56;

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

}  // namespace th_rt

struct th_model {
    int device = 0;
    int ncu = 0;                  // CUs of `device`: the persistent kernels size their grids by it
    unsigned flags = 0;
    hipStream_t stream = nullptr;
    std::vector<th_rt::Node> nodes;
    std::vector<const float*> blob_host;  // into `pack`
    std::vector<size_t> blob_count;
    std::vector<char> pack;
    std::vector<float*> dev_allocs;  // weights & derived tensors (freed by ~th_model)
    std::vector<th_rt::Buffer> bufs;
    std::vector<th_rt::Step> steps;
    int wino_v_buf = -1, wino_m_buf = -1;   // scratch arenas of the Winograd layers (shared: the layers run one after the other)
    ThKnobs knobs;                          // the TH_* knobs as th_model_load found them (plans and launchers point here)
    struct Guard {                          // load-time guard: written by guard_check (guard.hip), read by th_model_guard_info
        int state = 0;                      // 0 not run (TH_GUARD=0, or no fast plan to check), 1 passed, 2 tripped (fast features dropped)
        double dlogit = 0, scale = 0;       // max |logit(fast) - logit(direct)| of the plan that is kept, max |logit(direct)|
        double ms = 0;                      // wall time of the check inside th_model_load
        double ref_load_ms = 0, run_ms = 0;
        std::string note;
    } guard;
    int input_node = -1, output_node = -1, logits_node = -1;
    int in_dims[4] = {0, 0, 0, 0};
    int n_classes = 0;
    int chunk = 1024;
    int chunk_alloc = 0;
    int profiling = 0;            // 0 off, 1 every step, 2 only the step with the most algorithmic FLOPs
    int dominant_step = -1;
    std::vector<hipEvent_t> ev_pool;
    double algo_flops = 0, exec_flops = 0;
    // ---- host-buffer pipeline (th_predict / th_predict_async, predict.hip) ----
    // frames travel host -> device in pieces of <= chunk frames through a ring of kRing device buffers on a copy
    // stream; piece g's kernels (model stream) wait for its copy, the copy into a ring slot waits for the kernels
    // that last read it; probabilities return through a pinned host buffer per ticket on a third stream.
    static constexpr int kRing = 3;
    static constexpr int kTickets = 4;
    struct Ticket {
        bool busy = false;
        bool waiting = false;     // a th_predict_wait call owns this slot right now
        hipEvent_t computed = nullptr, done = nullptr;
        float* d_out = nullptr;  size_t d_out_floats = 0;
        float* h_out = nullptr;  size_t h_out_floats = 0;   // pinned
        float* user_out = nullptr;
        size_t floats = 0;
    };
    struct HostPipe {
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
        Ticket tickets[kTickets];
    } pipe;
    int64_t last_n = 0;
    const void* cur_in = nullptr;  // caller's frames for the chunk in flight (first-layer kernel reads them directly)
    int cur_dtype = TH_F32;
    bool need_convert = true;      // some consumer of the input needs the fp32 arena copy

    // ---- two lanes (TH_LANES=2): a chunk is cut in two halves that travel through the plan on two
    // streams, the second one a few steps behind the first, each in its own half of every arena.  Layers of different
    // kind then overlap on the device: an HBM-bound 1x1x1 layer (<= 24 KB of LDS, 4-wave workgroups) of one half co-resides
    // with the single 138 KB / 8-wave workgroup per CU of an MFMA-bound 10^3 growth convolution of the other half and runs
    // in its barrier / LDS-write / epilogue gaps, and vice versa.
    struct Lanes {
        int lanes = 1;
        int lag = 1;                  // steps the second lane runs behind the first at issue time
        hipStream_t stream2 = nullptr;
        hipEvent_t ev_fork = nullptr, ev_join = nullptr;
        int64_t off = 0;              // frame offset (inside the arenas) of the lane whose steps are being issued
    } lane;

    ~th_model();                  // drains the four streams, then releases everything the handle owns (runtime.hip)

    TView view(int node) const {
        const th_rt::Node& nd = nodes[node];
        TView v;
        const th_rt::Buffer& b = bufs[nd.buf];
        v.p = b.dev + lane.off * b.floats_per_frame;
        v.D = nd.D; v.H = nd.H; v.W = nd.W; v.C = nd.C;
        v.cs = nd.cs; v.coff = nd.coff; v.fs = b.floats_per_frame;
        v.blk = nd.blk;
        return v;
    }
};

namespace th_rt {
int cached_malloc(void** out, size_t bytes, int device);                    // devcache.hip
void cached_free(void* p);
int upload(th_model* m, const float* h, size_t count, float** out);         // planner.hip
int parse_pack(th_model* m);
int plan(th_model* m);
int ensure_buffers(th_model* m);                                            // predict.hip
int run_device(th_model* m, const void* d_frames, int dtype, int64_t n, float* d_probs, unsigned flags, bool sync = true);
int load_common(th_model* m, const ThKnobs& knobs);                         // runtime.hip
// guard.hip: *mp is the freshly loaded plan; on return it may have been replaced by a plan with fewer fast features
int guard_check(std::unique_ptr<th_model>* mp, std::function<std::unique_ptr<th_model>(const ThKnobs&, int*)> reload);
}  // namespace th_rt
