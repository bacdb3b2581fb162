// Load-time guard: guard_check, called by th_model_load_mem on every fresh plan.
// The default plan computes most layers in a minimal-filtering form (conv_wino / conv_wfused / k_conv_first_w) and the 5^3 GEMMs
// with bf16x3-split operands.  Their error was measured on the synthetic benchmark weights only; real `.h5` weights have never
// been seen here (reference predict.py:121), and parity is unpinned against TensorFlow.  So every load checks its own plan: a
// second, DIRECT plan of the same pack (fp32-input MFMA kernels only: TH_WINOGRAD=0 TH_WFUSED=0 TH_FIRST_WINO=0) runs a handful
// of internally generated frames, and the logits of the two plans must agree to kGuardTol x max(1, max |logit|).  If they do
// not, fast features are dropped in the order split GEMM -> 5^3 Winograd -> fused 10^3 Winograd -> first-layer F(2,3) until
// they do (the last step IS the direct plan).  th_model_guard_info reports what happened; TH_GUARD=0 switches the check off,
// TH_GUARD_TOL overrides the tolerance (tests force a trip with it).
#include "model.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>

#include <dlfcn.h>
#include <sys/stat.h>
#include <unistd.h>

using namespace th_rt;

namespace {

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

}  // namespace

int th_rt::guard_check(std::unique_ptr<th_model>* mp, std::function<std::unique_ptr<th_model>(const ThKnobs&, int*)> reload) {
    th_model* m = mp->get();
    if (!m->knobs.guard || !has_fast_steps(m)) return TH_OK;
    double tol = kGuardTol;
    if (const char* e = getenv("TH_GUARD_TOL")) tol = atof(e);        // read at load like every other knob (tests)
    const std::string key = guard_key(m, tol);
    {
        std::lock_guard<std::mutex> lock(g_guard_mu);
        auto it = g_guard_seen.find(key);
        if (it != g_guard_seen.end()) {
            m->guard.state = 1; m->guard.dlogit = it->second.dlogit; m->guard.scale = it->second.scale;
            m->guard.note = "(verdict of an earlier load of this pack in this process)";
            return TH_OK;
        }
    }
    std::string disk_key;
    const std::string disk_path = guard_disk_path(m, key, &disk_key);
    if (!disk_path.empty()) {
        GuardSeen seen;
        if (guard_disk_lookup(disk_path, disk_key, &seen)) {
            m->guard.state = 1; m->guard.dlogit = seen.dlogit; m->guard.scale = seen.scale;
            m->guard.note = "(verdict of an earlier process: " + disk_path + ")";
            std::lock_guard<std::mutex> lock(g_guard_mu);
            if (g_guard_seen.size() < 256) g_guard_seen[key] = seen;
            return TH_OK;
        }
    }
    const Node& in = m->nodes[m->input_node];
    std::vector<float> hf;
    guard_frames(&hf, (size_t)kGuardFrames * in.D * in.H * in.W * in.C);
    struct Scratch { float *frames = nullptr, *out = nullptr; ~Scratch() { cached_free(frames); cached_free(out); } } sc;
    int rc;
    if ((rc = cached_malloc((void**)&sc.frames, hf.size() * sizeof(float), m->device))) return rc;
    if ((rc = cached_malloc((void**)&sc.out, (size_t)kGuardFrames * 4096 * sizeof(float), m->device))) return rc;
    if (m->nodes[m->output_node].C > 4096 || (m->logits_node >= 0 && m->nodes[m->logits_node].C > 4096)) return TH_OK;
    {
        const hipError_t e = hipMemcpy(sc.frames, hf.data(), hf.size() * sizeof(float), hipMemcpyHostToDevice);
        if (e != hipSuccess) { th_set_error("guard: frame upload failed: %s", hipGetErrorString(e)); return TH_EHIP; }
    }
    ThKnobs direct = m->knobs;
    direct.guard = 0; direct.wino_split = 0; direct.first_split = 0; direct.wf_split = 0; direct.winograd = 0; direct.wfused = 0; direct.first_wino = 0;
    int lrc = TH_OK;
    const auto t0 = std::chrono::steady_clock::now();
    const std::unique_ptr<th_model> ref = reload(direct, &lrc);
    if (!ref) return lrc;
    const auto t1 = std::chrono::steady_clock::now();
    m->guard.ref_load_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    std::vector<float> want, got;
    if ((rc = guard_run(ref.get(), sc.frames, sc.out, &want))) return rc;
    m->guard.run_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
    double scale = 0;
    for (float v : want) scale = std::max(scale, (double)std::fabs(v));
    auto diff_of = [&](th_model* x, double* d) -> int {
        int r = guard_run(x, sc.frames, sc.out, &got);
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
    if ((rc = diff_of(m, &d))) return rc;
    m->guard.scale = scale;
    if (d <= bound) {
        m->guard.state = 1; m->guard.dlogit = d;
        guard_disk_store(disk_path, disk_key, {d, scale});
        std::lock_guard<std::mutex> lock(g_guard_mu);
        if (g_guard_seen.size() < 256) g_guard_seen[key] = {d, scale};
        return TH_OK;
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
        std::unique_ptr<th_model> alt = reload(k, &lrc);
        if (!alt) return lrc;
        double da = 0;
        if ((rc = diff_of(alt.get(), &da))) return rc;
        snprintf(note, sizeof note, "; %s %.3g", names[stage], da);
        hist += note;
        if (da <= bound || stage == kStages - 1) {
            alt->knobs.guard = m->knobs.guard;
            alt->guard.state = 2; alt->guard.dlogit = da; alt->guard.scale = scale;
            alt->guard.ref_load_ms = m->guard.ref_load_ms; alt->guard.run_ms = m->guard.run_ms;
            snprintf(note, sizeof note, "guard tripped (bound %.3g): ", bound);
            alt->guard.note = std::string(note) + hist + " -> kept with " + dropped;
            alt->knobs.nondefault += (alt->knobs.nondefault.empty() ? "" : " ") + std::string("guard:") + dropped;
            *mp = std::move(alt);
            return TH_OK;
        }
    }
    // No alternative was accepted: every fast feature was already off in the caller's knobs, so the plan IS the direct plan up to
    // kernels the guard does not switch — and it still differs from the reference plan by more than the bound.  Never report that
    // as a pass: the handle is usable, says "tripped" and carries the measured distance.
    m->guard.state = 2; m->guard.dlogit = d;
    snprintf(note, sizeof note, "guard tripped (bound %.3g): ", bound);
    m->guard.note = std::string(note) + hist + " -> no fast feature left to drop; plan kept as loaded";
    return TH_OK;
}
