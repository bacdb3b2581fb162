// Model runtime: errors, the TH_* knobs, model load / free, and what of the C ABI has no unit of its own (model.h lists the units).
//
// Replaces, behind include/timed_hip.h:
//   tf.keras.models.load_model(path)      reference predict.py:121  -> th_model_load
//   frame_model.predict(X_batch)          reference predict.py:142  -> th_predict / th_predict_device
#include "model.h"

#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstring>

using namespace th_rt;

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
    flag("TH_CONV_NOTAIL", &k->conv_notail);
    KNOCK("TH_CONV_DBG", conv_dbg);
    num("TH_N16_RESIDENT", &k->n16_resident, 0, 1 << 20);
    num("TH_PW_RESIDENT", &k->pw_resident, 0, 1 << 20);
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

int th_rt::load_common(th_model* m, const ThKnobs& knobs) {
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipDeviceGetAttribute(&m->ncu, hipDeviceAttributeMultiprocessorCount, m->device));
    HIP_TRY(hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&m->pipe.copy_stream, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&m->pipe.d2h_stream, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&m->lane.stream2, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&m->lane.ev_fork, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&m->lane.ev_join, hipEventDisableTiming));
    m->knobs = knobs;       // every A/B / test knob of this handle: the environment as th_model_load_mem read it, or the load-time guard's
    m->lane.lanes = m->knobs.lanes; m->lane.lag = m->knobs.lane_lag;
    for (int r = 0; r < th_model::kRing; ++r) {
        HIP_TRY(hipEventCreateWithFlags(&m->pipe.ev_h2d[r], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&m->pipe.ev_free[r], hipEventDisableTiming));
    }
    for (th_model::Ticket& t : m->pipe.tickets) {
        HIP_TRY(hipEventCreateWithFlags(&t.computed, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&t.done, hipEventDisableTiming));
    }
    int rc = parse_pack(m);
    if (rc) return rc;
    return plan(m);
}

th_model::~th_model() {
    (void)hipSetDevice(device);
    // queued kernels and copies may still read the arenas: drain the four streams before anything is released
    if (stream) (void)hipStreamSynchronize(stream);
    if (pipe.copy_stream) (void)hipStreamSynchronize(pipe.copy_stream);
    if (pipe.d2h_stream) (void)hipStreamSynchronize(pipe.d2h_stream);
    if (lane.stream2) (void)hipStreamSynchronize(lane.stream2);
    for (float* p : dev_allocs) cached_free(p);
    for (Buffer& b : bufs) if (b.dev) cached_free(b.dev);
    for (int r = 0; r < th_model::kRing; ++r) {
        if (pipe.d_in_ring[r]) cached_free(pipe.d_in_ring[r]);
        if (pipe.d_sp_ring[r]) cached_free(pipe.d_sp_ring[r]);
        if (pipe.ev_h2d[r]) (void)hipEventDestroy(pipe.ev_h2d[r]);
        if (pipe.ev_free[r]) (void)hipEventDestroy(pipe.ev_free[r]);
    }
    for (th_model::Ticket& t : pipe.tickets) {
        if (t.d_out) cached_free(t.d_out);
        if (t.h_out) (void)hipHostFree(t.h_out);
        if (t.computed) (void)hipEventDestroy(t.computed);
        if (t.done) (void)hipEventDestroy(t.done);
    }
    if (lane.stream2) (void)hipStreamDestroy(lane.stream2);
    if (lane.ev_fork) (void)hipEventDestroy(lane.ev_fork);
    if (lane.ev_join) (void)hipEventDestroy(lane.ev_join);
    if (pipe.copy_stream) (void)hipStreamDestroy(pipe.copy_stream);
    if (pipe.d2h_stream) (void)hipStreamDestroy(pipe.d2h_stream);
    for (hipEvent_t e : ev_pool) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
}

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
    if (rc) return rc;
    auto reload = [&](const ThKnobs& k, int* lrc) {                       // another plan of the same pack under other knobs
        std::unique_ptr<th_model> x(new th_model);
        x->device = device;
        x->flags = flags;
        x->pack.assign((const char*)pack, (const char*)pack + nbytes);
        *lrc = load_common(x.get(), k);
        if (*lrc) x.reset();
        return x;
    };
    const auto g0 = std::chrono::steady_clock::now();
    rc = guard_check(&m, reload);
    if (rc) return rc;
    m->guard.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - g0).count();
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

void th_model_free(th_model* m) { delete m; }

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
    if (state) *state = m->guard.state;
    if (max_dlogit) *max_dlogit = m->guard.dlogit;
    if (logit_scale) *logit_scale = m->guard.scale;
    if (note && note_len) {
        if (m->guard.state == 0) snprintf(note, note_len, "%s", m->guard.note.c_str());
        else snprintf(note, note_len, "%s%s[%.1f ms: direct plan load %.1f, its run %.1f]", m->guard.note.c_str(), m->guard.note.empty() ? "" : " ",
                      m->guard.ms, m->guard.ref_load_ms, m->guard.run_ms);
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
