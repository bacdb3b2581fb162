// Executor (ensure_buffers, run_device) and the host-buffer pipeline behind th_predict*: copy ring, tickets, sparse transport.
#include "model.h"

#include <algorithm>
#include <cstring>

using namespace th_rt;

int th_rt::ensure_buffers(th_model* m) {
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

static size_t dtype_size(int dt) {
    switch (dt) {
        case TH_F32: return 4;
        case TH_F64: return 8;
        case TH_U8: case TH_BOOL: return 1;
        case TH_F16: return 2;
        default: return 0;
    }
}

int th_rt::run_device(th_model* m, const void* d_frames, int dtype, int64_t n, float* d_probs, unsigned flags, bool sync) {
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
        const bool two = m->lane.lanes == 2 && !m->profiling && cnt >= 256 && m->lane.stream2;
        if (two) {
            // halves of the chunk on two streams; lane 1 issues `lane_lag` steps behind lane 0
            const int64_t h0 = (cnt / 2 + 63) / 64 * 64, h1 = cnt - h0;
            const char* in0 = (const char*)m->cur_in;
            HIP_TRY(hipEventRecord(m->lane.ev_fork, m->stream));
            HIP_TRY(hipStreamWaitEvent(m->lane.stream2, m->lane.ev_fork, 0));
            std::vector<size_t> order;
            for (size_t si = 0; si < m->steps.size(); ++si)
                if (!(logits && m->steps[si].is_final_softmax)) order.push_back(si);
            const int L = std::max(0, m->lane.lag);
            for (size_t k = 0; k < order.size() + (size_t)L; ++k) {
                if (k < order.size()) {
                    m->lane.off = 0; m->cur_in = in0;
                    if ((rc = m->steps[order[k]].run(m->stream, h0))) { m->lane.off = 0; return rc; }
                }
                if (k >= (size_t)L) {
                    m->lane.off = h0; m->cur_in = in0 + (size_t)h0 * frame_bytes;
                    rc = m->steps[order[k - L]].run(m->lane.stream2, h1);
                    m->lane.off = 0; m->cur_in = in0;
                    if (rc) return rc;
                }
            }
            m->lane.off = 0; m->cur_in = in0;
            HIP_TRY(hipEventRecord(m->lane.ev_join, m->lane.stream2));
            HIP_TRY(hipStreamWaitEvent(m->stream, m->lane.ev_join, 0));
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

extern "C" {

int th_predict_device(th_model* m, const void* d_frames, int dtype, int64_t n, float* d_probs, unsigned flags) {
    if (n < 0) TH_FAIL(TH_EINVAL, "negative frame count");
    if (!m || (n > 0 && (!d_frames || !d_probs))) TH_FAIL(TH_EINVAL, "null argument");
    std::lock_guard<std::mutex> lock(m->pipe.mu);
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
    std::lock_guard<std::mutex> lock(m->pipe.mu);
    int rc = predict_async_locked(m, frames, dtype, n, probs_out, flags, ticket);
    if (rc) {
        // part of the batch may already be queued: nothing of it may still read the caller's frames (or write a ticket
        // buffer the next submission reallocates) once the error has been returned
        const std::string keep = th_last_error();
        (void)hipStreamSynchronize(m->pipe.copy_stream);
        (void)hipStreamSynchronize(m->stream);
        (void)hipStreamSynchronize(m->pipe.d2h_stream);
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
    for (int k = 0; k < th_model::kTickets; ++k) if (!m->pipe.tickets[k].busy) { ti = k; break; }
    if (ti < 0) TH_FAIL(TH_EBUSY, "all %d tickets of this model are in flight: call th_predict_wait first", th_model::kTickets);
    th_model::Ticket& t = m->pipe.tickets[ti];
    // A batch that fits one chunk is NOT cut further: measured, 125-frame pieces under-fill the 256 CUs and lose
    // more than the overlap wins.  Overlap across small batches comes from submitting the next ticket early.
    const int64_t piece = std::min<int64_t>(m->chunk, std::max<int64_t>(n, 1));
    const size_t need_in = frame_bytes * (size_t)piece;
    if (!(flags & TH_PREDICT_IN_DEVICE) && m->pipe.in_ring_bytes < need_in) {
        // growing the ring: nothing may still be reading the old buffers
        HIP_TRY(hipStreamSynchronize(m->pipe.copy_stream));
        HIP_TRY(hipStreamSynchronize(m->stream));
        for (int r = 0; r < th_model::kRing; ++r) {
            if (m->pipe.d_in_ring[r]) cached_free(m->pipe.d_in_ring[r]);
            m->pipe.d_in_ring[r] = nullptr;
            m->pipe.ring_used[r] = false;
        }
        m->pipe.in_ring_bytes = 0;
        for (int r = 0; r < th_model::kRing; ++r)
            if (int rc = cached_malloc(&m->pipe.d_in_ring[r], need_in, m->device)) return rc;
        m->pipe.in_ring_bytes = need_in;
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
        const int r = (int)(m->pipe.piece_counter % th_model::kRing);
        if (m->pipe.ring_used[r]) {
            // the kernels of the piece that used this ring buffer three pieces ago must have finished with it
            if (pinned) HIP_TRY(hipStreamWaitEvent(m->pipe.copy_stream, m->pipe.ev_free[r], 0));
            else HIP_TRY(hipEventSynchronize(m->pipe.ev_free[r]));
        }
        if (sp) {
            // sparse transport: the piece's bitmaps, ranks and stored values travel (a tenth of the dense bytes for Gaussian frames);
            // k_sparse_expand rebuilds the dense frames in the ring buffer, on the compute stream, in front of the first layer
            const size_t bits_b = (size_t)cnt * sp->W * 4, vidx_b = (size_t)(cnt + 1) * 8;
            const uint64_t v0 = sp->vidx[off], v1 = sp->vidx[off + cnt];
            const size_t val_b = (size_t)(v1 - v0) * 4;
            const size_t o_vidx = (bits_b + 15) / 16 * 16, o_val = (o_vidx + vidx_b + 15) / 16 * 16, need = o_val + val_b + 16;
            if (m->pipe.sp_ring_bytes < need) {
                HIP_TRY(hipStreamSynchronize(m->pipe.copy_stream));
                HIP_TRY(hipStreamSynchronize(m->stream));
                for (int q = 0; q < th_model::kRing; ++q) {
                    if (m->pipe.d_sp_ring[q]) cached_free(m->pipe.d_sp_ring[q]);
                    m->pipe.d_sp_ring[q] = nullptr;
                }
                m->pipe.sp_ring_bytes = 0;
                const size_t cap = need + need / 4;
                for (int q = 0; q < th_model::kRing; ++q)
                    if (int rc = cached_malloc(&m->pipe.d_sp_ring[q], cap, m->device)) return rc;
                m->pipe.sp_ring_bytes = cap;
            }
            char* const d = (char*)m->pipe.d_sp_ring[r];
            HIP_TRY(hipMemcpyAsync(d, sp->bits + (size_t)off * sp->W, bits_b, hipMemcpyHostToDevice, m->pipe.copy_stream));
            HIP_TRY(hipMemcpyAsync(d + o_vidx, sp->vidx + off, vidx_b, hipMemcpyHostToDevice, m->pipe.copy_stream));
            if (val_b) HIP_TRY(hipMemcpyAsync(d + o_val, sp->values + (v0 - sp->vidx[0]), val_b, hipMemcpyHostToDevice, m->pipe.copy_stream));
            HIP_TRY(hipEventRecord(m->pipe.ev_h2d[r], m->pipe.copy_stream));
            HIP_TRY(hipStreamWaitEvent(m->stream, m->pipe.ev_h2d[r], 0));
            int rc = launch_sparse_expand(m->stream, cnt, (const uint32_t*)d, (const uint64_t*)(d + o_vidx), (const float*)(d + o_val),
                                          (float*)m->pipe.d_in_ring[r], sp->E, sp->W);
            if (rc) return rc;
        } else {
        HIP_TRY(hipMemcpyAsync(m->pipe.d_in_ring[r], (const char*)frames + (size_t)off * frame_bytes, (size_t)cnt * frame_bytes,
                               hipMemcpyHostToDevice, m->pipe.copy_stream));
        HIP_TRY(hipEventRecord(m->pipe.ev_h2d[r], m->pipe.copy_stream));
        HIP_TRY(hipStreamWaitEvent(m->stream, m->pipe.ev_h2d[r], 0));
        }
        int rc = run_device(m, m->pipe.d_in_ring[r], dtype, cnt, (out_on_device ? probs_out : t.d_out) + (size_t)off * width, flags,
                            /*sync=*/false);
        if (rc) return rc;
        HIP_TRY(hipEventRecord(m->pipe.ev_free[r], m->stream));
        m->pipe.ring_used[r] = true;
        m->pipe.piece_counter++;
    }
    HIP_TRY(hipEventRecord(t.computed, m->stream));
    HIP_TRY(hipStreamWaitEvent(m->pipe.d2h_stream, t.computed, 0));
    if (floats && !out_on_device)
        HIP_TRY(hipMemcpyAsync(t.h_out, t.d_out, floats * sizeof(float), hipMemcpyDeviceToHost, m->pipe.d2h_stream));
    HIP_TRY(hipEventRecord(t.done, m->pipe.d2h_stream));
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
    std::lock_guard<std::mutex> lock(m->pipe.mu);
    int rc = predict_async_locked(m, blob, TH_F32, n32, probs_out, flags, ticket, &sp);
    if (rc) {
        const std::string keep = th_last_error();
        (void)hipStreamSynchronize(m->pipe.copy_stream);
        (void)hipStreamSynchronize(m->stream);
        (void)hipStreamSynchronize(m->pipe.d2h_stream);
        (void)hipGetLastError();
        th_set_error("%s", keep.c_str());
    }
    return rc;
}

int th_predict_wait(th_model* m, int ticket) {
    if (!m || ticket < 0 || ticket >= th_model::kTickets) TH_FAIL(TH_EINVAL, "bad ticket");
    th_model::Ticket& t = m->pipe.tickets[ticket];
    {
        std::lock_guard<std::mutex> lock(m->pipe.mu);
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
    std::lock_guard<std::mutex> lock(m->pipe.mu);
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

}  // extern "C"
