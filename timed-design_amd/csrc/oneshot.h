// Host scaffolding of the one-shot entry points (th_superpose, th_lddt, th_tmscore, ...): a call validates its arguments, lays one
// device allocation out, opens a scope, copies in, launches, copies out and returns; whatever it holds on the device goes with the
// scope on every return path.  Four plain pieces and no driver: the entry point itself stays the list of HIP calls, top to bottom.
#pragma once
#include <climits>
#include <new>
#include <vector>

#include "common.h"

// Byte offsets inside the call's one allocation: every array starts on a 256-byte boundary.
struct ThLayout {
    size_t bytes = 0;
    size_t take(size_t b) { const size_t at = bytes; bytes += (b + 255) & ~(size_t)255; return at; }
};

// hipMalloc through th_malloc_retry; a failure leaves *mem NULL and its text in th_last_error (TH_ENOMEM when the device is full)
inline int th_alloc_or_fail(const char* who, unsigned char** mem, size_t bytes) {
    hipError_t e = th_malloc_retry(mem, bytes);
    if (e == hipSuccess) return TH_OK;
    (void)hipGetLastError();
    *mem = nullptr;
    th_set_error("%s: hipMalloc of %zu bytes: %s", who, bytes, hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? TH_ENOMEM : TH_EHIP;
}

// What one call owns on the device.  Nothing is released before every stream has drained.
struct ThCall {
    int device = -1;
    hipStream_t st[2] = {nullptr, nullptr};
    unsigned char* mem[2] = {nullptr, nullptr};
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    ThCall() = default;
    ThCall(const ThCall&) = delete;
    ThCall& operator=(const ThCall&) = delete;
    ~ThCall() {
        if (device < 0) return;
        (void)hipSetDevice(device);
        for (hipStream_t s : st)
            if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        for (unsigned char* m : mem)
            if (m) (void)hipFree(m);
    }
    // the device, mem[0] of `bytes` and 256 more (never a zero-byte allocation), st[0], and n_events events (0: the caller wants no times)
    int open(const char* who, int device, size_t bytes, int n_events) {
        HIP_TRY(hipSetDevice(device));
        this->device = device;
        if (int rc = th_alloc_or_fail(who, &mem[0], bytes + 256)) return rc;
        HIP_TRY(hipStreamCreateWithFlags(&st[0], hipStreamNonBlocking));
        for (int i = 0; i < n_events; ++i) HIP_TRY(hipEventCreate(&ev[i]));
        return TH_OK;
    }
    template <class T> T* at(size_t offset) const { return reinterpret_cast<T*>(mem[0] + offset); }
    hipError_t mark(int i) { return ev[i] ? hipEventRecord(ev[i], st[0]) : hipSuccess; }
    // waits for st[0]; kernel_ms[q] = milliseconds from mark(q) to mark(q + 1)
    int finish(double* kernel_ms, int spans = 1) {
        HIP_TRY(hipStreamSynchronize(st[0]));
        for (int q = 0; kernel_ms && q < spans; ++q) {
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, ev[q], ev[q + 1]));
            kernel_ms[q] = ms;
        }
        return TH_OK;
    }
};

// offsets[0 .. n] of n consecutive ranges: from 0 to total, never decreasing
inline int th_check_offsets(const char* who, const char* name, const char* total_name, const int64_t* offsets, int64_t n, int64_t total) {
    if (offsets[0] != 0 || offsets[n] != total)
        TH_FAIL(TH_EINVAL, "%s: %s run from %lld to %lld, not from 0 to %s = %lld", who, name, (long long)offsets[0], (long long)offsets[n],
                total_name, (long long)total);
    for (int64_t p = 0; p < n; ++p)
        if (offsets[p + 1] < offsets[p]) TH_FAIL(TH_EINVAL, "%s: %s[%lld] > %s[%lld]", who, name, (long long)p, name, (long long)p + 1);
    return TH_OK;
}

// A work item of the kernels that stream a range past a tile of it: elements offsets[range] + tile * length ... of that range.
struct ThTile { int range, tile; };

// items: one per started tile of `length` elements of each of the n ranges of offsets, in range order; `what` names the elements
inline int th_tile_items(const char* who, const char* what, const int64_t* offsets, int64_t n, int64_t length, std::vector<ThTile>& items) {
    try {
        items.reserve((size_t)(offsets[n] / length + (n < offsets[n] ? n : offsets[n])));      // a range with elements has one partial tile at most
        for (int64_t r = 0; r < n; ++r) {
            const int64_t tiles = (offsets[r + 1] - offsets[r] + length - 1) / length;
            for (int64_t t = 0; t < tiles; ++t) items.push_back(ThTile{(int)r, (int)t});
        }
    } catch (const std::bad_alloc&) {
        TH_FAIL(TH_ENOMEM, "%s: out of host memory for the work items of %lld %s", who, (long long)offsets[n], what);
    }
    if (items.size() > (size_t)INT_MAX) TH_FAIL(TH_EINVAL, "%s: %zu work items in one call (limit 2^31 - 1)", who, items.size());
    return TH_OK;
}
