// Per-process device block cache.
// predict.py loads and frees a model per call (the reference does: predict.py:114-121); a TIMED handle is ~50 device blocks —
// weights, activation arenas, rings — and hipFree synchronises the device each time: 13 ms per close, 10 ms per load.  Blocks a
// model gives back are kept here (exact-size reuse, at most kCacheBytes per process) and returned to HIP by th_dev_trim or when
// the cap is reached.  Callers synchronise the streams that used a block before they release it.
#include "model.h"

#include <algorithm>
#include <map>

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
}  // namespace

int th_rt::cached_malloc(void** out, size_t bytes, int device) {
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

void th_rt::cached_free(void* p) {
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
