#pragma once
// Runtime layer of the MI355X BBS+ engine (included by every translation unit): contexts (device-resident tables), jobs
// (device-resident batches), validation in the reference's order, kernel launches on the
// context's HIP stream.  See include/bbs_sign_amd.h for the contract.
//
// Build: hipcc --offload-arch=gfx950 (product, libbbs_sign_amd.so).  The macro BBS_HOST_TWIN
// (tests/hosttwin only, never part of the product library) swaps the HIP runtime calls for
// malloc/memcpy/for-loops so that the host logic in this file can be unit-tested in a container
// without a GPU; the product build contains no CPU execution path for the stages.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <cstring>
#include <functional>
#include <iterator>
#include <map>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <memory>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/bbs_sign_amd.h"
#include "host_g2.hpp"
#include "codec_dev.hpp"
#include "keyed.hpp"
#include "queue_policy.hpp"
#include "key_cache.hpp"

using namespace bbs;

// =============================================================================================
// runtime layer
// =============================================================================================
namespace rt {
// What the library found when it was loaded (capi.hip's constructor records it before it writes its own GPU_MAX_HW_QUEUES): was
// the variable there, and had the HIP runtime -- which reads it once, at its own initialisation -- already started.  From the
// two, the pool the runtime most probably uses (queue_policy.hpp load_pool); never recorded = the runtime's default.
struct LoadState { bool recorded = false, variable_was_set = false; int value_found = 0, runtime_at_load = qpolicy::RT_UNKNOWN; };
inline LoadState& load_state() { static LoadState s; return s; }
inline int effective_pool() {
    const LoadState& s = load_state();
    return s.recorded ? qpolicy::load_pool(s.variable_was_set, s.value_found, s.runtime_at_load) : qpolicy::RUNTIME_POOL;
}
// The dedicated-queue setting of the process: -2 not decided yet (BBS_DEDICATED_QUEUES is read when it is first needed),
// qpolicy::AUTO (-1) nothing was asked for, 0 off, k > 0 up to k job streams per device
inline std::atomic<int>& dedicated_queues() { static std::atomic<int> v{-2}; return v; }
inline int dedicated_setting() {
    int want = dedicated_queues().load();
    if (want < qpolicy::AUTO) {
        const char* e = getenv("BBS_DEDICATED_QUEUES");
        want = e && *e ? atoi(e) : qpolicy::AUTO;
        if (e && *e) { if (want == 1) want = 12; if (want < 0) want = 0; if (want > qpolicy::MAX_DEDICATED) want = qpolicy::MAX_DEDICATED; }
        int undecided = -2;
        if (!dedicated_queues().compare_exchange_strong(undecided, want)) want = undecided;      // bbs_runtime_set_dedicated_queues came first
    }
    return want;
}
#ifdef BBS_HOST_TWIN
struct Stream {};
inline int set_device(int) { return 0; }
inline int device_count() { return 1; }
inline int stream_create(Stream*) { return 0; }
inline void stream_destroy(Stream&) {}
struct QueueBudget { int total = 0, pool = 0, dedicated_cap = 0; size_t scratch = 0; };
inline QueueBudget queue_budget(int) { return QueueBudget{}; }
inline void queue_counts(int, int* dedicated, int* pooled) { *dedicated = 0; *pooled = 0; }
inline size_t size_class(size_t b) { return b; }
inline int dmalloc(void** p, size_t b) { *p = std::calloc(b ? b : 1, 1); return *p ? 0 : -1; }
inline void dfree(void* p, size_t, int) { std::free(p); }
inline int current_device() { return 0; }
inline int h2d(void* d, const void* h, size_t b, Stream&) { if (b) std::memcpy(d, h, b); return 0; }
inline int d2h(void* h, const void* d, size_t b, Stream&) { if (b) std::memcpy(h, d, b); return 0; }
inline int dmemset(void* d, int v, size_t b, Stream&) { if (b) std::memset(d, v, b); return 0; }
inline int d2d_async(void* d, const void* s, size_t b, Stream&) { if (b) std::memcpy(d, s, b); return 0; }
inline int h2d_async(void* d, const void* h, size_t b, Stream&) { if (b) std::memcpy(d, h, b); return 0; }
inline int d2h_async(void* h, const void* d, size_t b, Stream&) { if (b) std::memcpy(h, d, b); return 0; }
inline int hmalloc(void** p, size_t b) { *p = std::malloc(b ? b : 1); return *p ? 0 : -1; }
inline void hfree(void* p, size_t) { std::free(p); }
inline int sync(Stream&) { return 0; }
inline size_t mem_free_bytes() { return (size_t)64 << 20; }      // test build: the automatic window width comes out as 8
struct Event { };
inline int event_create(Event*) { return 0; }
inline void event_destroy(Event&) {}
inline int event_record(Event&, Stream&) { return 0; }
inline int stream_wait(Stream&, Event&) { return 0; }
inline bool event_done(Event&) { return true; }
template <class F, class A>
inline int launch(Stream&, const A& a, size_t nthreads) {
    for (size_t t = 0; t < nthreads; t++) F::run(a, t);
    return 0;
}
// a list of time stamps recorded on the stream; read back after one synchronisation
struct EventList {
    std::vector<std::chrono::steady_clock::time_point> t;
    size_t used = 0;
    explicit EventList(size_t) {}
    int record(Stream&) { t.push_back(std::chrono::steady_clock::now()); used++; return 0; }
    int finish(Stream&) { return 0; }
    float ms(size_t a, size_t b) { return std::chrono::duration<float, std::milli>(t[b] - t[a]).count(); }
};
#else
using Stream = hipStream_t;
inline int set_device(int d) { return hipSetDevice(d) == hipSuccess ? 0 : -1; }
inline int device_count() { int n = 0; return hipGetDeviceCount(&n) == hipSuccess ? n : 0; }
inline int stream_create(Stream* s);      // pooled, defined below
inline void stream_destroy(Stream& s);
// Device buffers, streams and events are recycled per device: a one-shot batch call allocated ~20 buffers and two
// streams and released them again, 6 ms of hipMalloc / hipFree / stream creation per 4096-proof call.  Buffers up
// to 256 MiB go back to a free list by size class (powers of two below 1 MiB, multiples of 1 MiB above), at most
// 8 GiB per device; larger ones (the window tables) are allocated and freed directly.
struct Pools {
    std::mutex mu;
    // a pooled buffer remembers WHEN it came back (`clock`): when the pool is full the buffers that have waited longest -- what
    // an earlier workload left behind -- make room, never the working set (round 5: evicting by size, smallest first, let
    // twelve 16384-item jobs' buffers sit in a full pool for ever while a later workload of smaller jobs paid hipMalloc /
    // hipFree -- a device synchronisation -- on every buffer: the issuer's lists at half their rate)
    struct Pooled { void* p; uint64_t seq; };
    uint64_t clock = 0;
    std::map<int, std::multimap<size_t, Pooled>> bufs;
    std::map<int, size_t> pooled_bytes;
    // streams: handed out in creation order (lowest creation index first), not last-freed-first.  The runtime binds a
    // stream to one of the GPU_MAX_HW_QUEUES hardware queues when it is created, round robin; a job's two streams
    // carry its two long kernels (MSM chain / pairing), and with last-in-first-out recycling some sequences of frees
    // put the pairing streams of a set of concurrent jobs on a few hardware queues (measured: 1.19 M instead of
    // 1.37 M proof_verify/s for the first eight jobs after 32 others were freed).  In creation order a set of jobs
    // created back to back gets the queue spread of freshly created streams.
    std::map<int, std::set<std::pair<uint64_t, hipStream_t>>> streams;
    std::map<hipStream_t, uint64_t> stream_index;
    uint64_t next_stream_index = 0;
    std::map<int, std::vector<hipEvent_t>> events;
    // page-locked host staging buffers (one per batch: raw inputs in, statuses out), by size class; hipHostMalloc
    // costs hundreds of microseconds, a batch call must not pay it
    std::multimap<size_t, Pooled> pinned;
    size_t pinned_bytes = 0;
    // the entry of `m` that has waited longest among the size classes other than `cls` (m.end(): there is none)
    template <class M> static typename M::iterator oldest_other(M& m, size_t cls) {
        auto best = m.end();
        for (auto it = m.begin(); it != m.end(); ++it)
            if (it->first != cls && (best == m.end() || it->second.seq < best->second.seq)) best = it;
        return best;
    }
    std::map<int, std::vector<hipEvent_t>> timing_events;      // events WITH timing (stage timers), recycled
    std::map<int, int> dedicated_made;                         // streams with a hardware queue of their own, per device
    std::map<int, int> pooled_made;                            // streams drawn from the runtime's GPU_MAX_HW_QUEUES pool, per device (alive or recycled here)
    std::set<hipStream_t> dedicated;                           // which of the recycled streams are the dedicated ones
    bool closing = false;                                      // the process is exiting: dedicated streams are destroyed, not recycled
    static Pools& get() { static Pools* p = new Pools(); return *p; }      // lives as long as the process
};
inline int current_device() { int d = 0; (void)hipGetDevice(&d); return d; }
inline size_t size_class(size_t b) {
    if (b < 256) return 256;
    if (b <= (1u << 20)) { size_t c = 256; while (c < b) c <<= 1; return c; }
    return (b + (1u << 20) - 1) & ~(size_t)((1u << 20) - 1);
}
constexpr size_t POOL_MAX_BUF = (size_t)256 << 20, POOL_MAX_TOTAL = (size_t)8 << 30;
inline int dmalloc(void** p, size_t b) {
    const size_t cls = size_class(b);
    if (cls <= POOL_MAX_BUF) {
        Pools& P = Pools::get();
        std::lock_guard<std::mutex> g(P.mu);
        auto& m = P.bufs[current_device()];
        auto it = m.find(cls);
        if (it != m.end()) { *p = it->second.p; m.erase(it); P.pooled_bytes[current_device()] -= cls; return 0; }
    }
    if (hipMalloc(p, cls) == hipSuccess) return 0;
    (void)hipGetLastError();      // an allocation that failed must not be reported again by the next launch's error check
    *p = nullptr;
    return -1;
}
inline void dfree(void* p, size_t b, int dev) {        // dev = the device the buffer was allocated on
    const size_t cls = size_class(b);
    std::vector<void*> evicted;
    if (cls <= POOL_MAX_BUF) {
        // as hfree: the size in use now is kept; when the pool is full, the buffers of other sizes that have waited longest make room
        Pools& P = Pools::get();
        std::lock_guard<std::mutex> g(P.mu);
        auto& m = P.bufs[dev];
        size_t& tot = P.pooled_bytes[dev];
        while (tot + cls > POOL_MAX_TOTAL && !m.empty()) {
            auto it = Pools::oldest_other(m, cls);
            if (it == m.end()) break;                          // only this size is cached: the pool is simply full of it
            evicted.push_back(it->second.p);
            tot -= it->first;
            m.erase(it);
        }
        if (tot + cls <= POOL_MAX_TOTAL) { m.emplace(cls, Pools::Pooled{p, ++P.clock}); tot += cls; p = nullptr; }
    }
    for (void* e : evicted) (void)hipFree(e);
    if (p) (void)hipFree(p);
}
inline int h2d(void* d, const void* h, size_t b, Stream& s) {
    if (!b) return 0;
    if (hipMemcpyAsync(d, h, b, hipMemcpyHostToDevice, s) != hipSuccess) return -1;
    return hipStreamSynchronize(s) == hipSuccess ? 0 : -1;   // host staging buffers are transient
}
inline int d2h(void* h, const void* d, size_t b, Stream& s) {
    if (!b) return 0;
    if (hipMemcpyAsync(h, d, b, hipMemcpyDeviceToHost, s) != hipSuccess) return -1;
    return hipStreamSynchronize(s) == hipSuccess ? 0 : -1;
}
inline int dmemset(void* d, int v, size_t b, Stream& s) { return (!b || hipMemsetAsync(d, v, b, s) == hipSuccess) ? 0 : -1; }
inline int d2d_async(void* d, const void* s_, size_t b, Stream& s) {
    return (!b || hipMemcpyAsync(d, s_, b, hipMemcpyDeviceToDevice, s) == hipSuccess) ? 0 : -1;
}
// asynchronous copies from / to page-locked staging memory (hmalloc): the caller keeps the host buffer alive until the
// stream has passed the copy
inline int h2d_async(void* d, const void* h, size_t b, Stream& s) {
    return (!b || hipMemcpyAsync(d, h, b, hipMemcpyHostToDevice, s) == hipSuccess) ? 0 : -1;
}
inline int d2h_async(void* h, const void* d, size_t b, Stream& s) {
    return (!b || hipMemcpyAsync(h, d, b, hipMemcpyDeviceToHost, s) == hipSuccess) ? 0 : -1;
}
constexpr size_t PINNED_POOL_MAX = (size_t)1 << 30;
inline int hmalloc(void** p, size_t b) {
    const size_t cls = size_class(b);
    {
        Pools& P = Pools::get();
        std::lock_guard<std::mutex> g(P.mu);
        auto it = P.pinned.find(cls);
        if (it != P.pinned.end()) { *p = it->second.p; P.pinned.erase(it); P.pinned_bytes -= cls; return 0; }
    }
    return hipHostMalloc(p, cls, hipHostMallocPortable) == hipSuccess ? 0 : -1;      // portable: the pool is shared by every device of the process
}
inline void hfree(void* p, size_t b) {
    const size_t cls = size_class(b);
    std::vector<void*> evicted;
    {
        // the buffer just released is the size the caller is using NOW: it is kept, and if the pool is full, buffers of
        // other sizes (left over from an earlier workload) make room -- otherwise a serving loop whose batch shape
        // changed would pay hipHostMalloc / hipHostFree (milliseconds) on every batch from then on
        Pools& P = Pools::get();
        std::lock_guard<std::mutex> g(P.mu);
        if (cls <= PINNED_POOL_MAX) {
            while (P.pinned_bytes + cls > PINNED_POOL_MAX && !P.pinned.empty()) {
                auto it = Pools::oldest_other(P.pinned, cls);
                if (it == P.pinned.end()) break;               // only this size is cached: the pool is simply full of it
                evicted.push_back(it->second.p);
                P.pinned_bytes -= it->first;
                P.pinned.erase(it);
            }
            if (P.pinned_bytes + cls <= PINNED_POOL_MAX) { P.pinned.emplace(cls, Pools::Pooled{p, ++P.clock}); P.pinned_bytes += cls; p = nullptr; }
        }
    }
    for (void* e : evicted) (void)hipHostFree(e);
    if (p) (void)hipHostFree(p);
}
inline int sync(Stream& s) { return hipStreamSynchronize(s) == hipSuccess ? 0 : -1; }
inline size_t mem_free_bytes() { size_t f = 0, t = 0; return hipMemGetInfo(&f, &t) == hipSuccess ? f : 0; }
using Event = hipEvent_t;
// ---- hardware queues x scratch: ONE budget, checked (round 5; DESIGN.md 5 rule 6) ---------------------------------------
// The runtime reserves scratch per hardware queue for every wave slot of the chip, sized for the largest kernel frame the
// queue has run: bytes per lane x 64 lanes x wave slots (8192 on MI355X).  Measured (profiles/r03_q_*, r04_g_*): up to
// queues x bytes/lane ~ 48 k everything runs, from ~ 50 k the runtime starts reclaiming scratch between dispatches and every
// rate collapses, from ~ 56 k it ABORTS THE PROCESS (HSA_STATUS_ERROR_OUT_OF_RESOURCES).  The library therefore knows its own
// largest kernel frame -- every kernel registers itself when the library is loaded, hipFuncGetAttributes gives the frame
// -- and never lets (pooled + dedicated) hardware queues x that frame exceed SCRATCH_POOL_FRACTION of the device's memory:
// dedicated queues beyond the budget are not created (the stream comes from the pool), and if the POOL alone is over budget
// (an explicit GPU_MAX_HW_QUEUES=32) the library stops creating streams at the budget -- a job that gets no stream of its
// own shares its context's stream (JobBase::stream) or runs its side streams' work on its main stream.  Slower, never an abort.
struct KernelRegistry {
    std::mutex mu;
    std::vector<const void*> fns;
    static KernelRegistry& get() { static KernelRegistry* r = new KernelRegistry(); return *r; }      // lives as long as the process
};
inline int register_kernel(const void* f) {
    KernelRegistry& r = KernelRegistry::get();
    std::lock_guard<std::mutex> g(r.mu);
    r.fns.push_back(f);
    return (int)r.fns.size();
}
// largest private segment (scratch bytes per lane) of any kernel of this library; once, after the runtime is up
inline size_t library_max_scratch() {
    static const size_t v = []() {
        KernelRegistry& r = KernelRegistry::get();
        std::lock_guard<std::mutex> g(r.mu);
        size_t m = 0;
        for (const void* f : r.fns) {
            hipFuncAttributes a;
            if (hipFuncGetAttributes(&a, f) == hipSuccess) m = std::max(m, (size_t)a.localSizeBytes);
            else (void)hipGetLastError();
        }
        return m;
    }();
    return v;
}
constexpr double SCRATCH_POOL_FRACTION = 0.085;       // of the device's memory: 26 GB of 288 GiB = 47 k (queues x bytes per lane)
struct QueueBudget {
    int total = 0;            // hardware queues (pooled + dedicated) the scratch budget allows
    int pool = 0;             // the runtime's pool: GPU_MAX_HW_QUEUES as the environment has it, 4 when unset
    int dedicated_cap = 0;    // dedicated queues the budget leaves room for: max(0, total - pool)
    size_t scratch = 0;       // bytes per lane of the library's largest kernel frame
};
inline QueueBudget queue_budget(int dev) {
    static std::mutex mu;
    static std::map<int, QueueBudget> cache;
    std::lock_guard<std::mutex> g(mu);
    auto it = cache.find(dev);
    if (it != cache.end()) return it->second;
    QueueBudget b;
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, dev) != hipSuccess) { (void)hipGetLastError(); return b; }
    b.scratch = library_max_scratch();
    const size_t wave_slots = (size_t)p.multiProcessorCount * (size_t)std::max(1, p.maxThreadsPerMultiProcessor / 64);
    const double per_queue = (double)std::max<size_t>(b.scratch, 64) * 64.0 * (double)wave_slots;
    b.total = (int)std::min(64.0, std::max(1.0, (double)p.totalGlobalMem * SCRATCH_POOL_FRACTION / per_queue));
    const char* v = getenv("GPU_MAX_HW_QUEUES");
    b.pool = v && atoi(v) > 0 ? atoi(v) : 4;
    b.dedicated_cap = std::max(0, b.total - b.pool);
    cache[dev] = b;
    return b;
}
// Dedicated streams do not outlive the process's exit handlers.  The runtime's own teardown destroys the hardware queues of
// its pool but not those of streams with a compute-unit mask that nobody destroyed, and a queue left behind is still known to
// whatever intercepts the queues of the process: under rocprofv3's kernel trace the profiler's exit-time destructor waited on
// the signal of each such queue after the runtime had gone -- a segmentation fault at the very end of a run whose output was
// complete.  So the first dedicated stream registers this handler (after the runtime's initialisation, hence run before its
// teardown): the dedicated streams waiting in the pool are destroyed, and those still in use are when they come back.
inline void release_dedicated_streams_at_exit() {
    Pools& P = Pools::get();
    std::vector<hipStream_t> gone;
    {
        std::lock_guard<std::mutex> g(P.mu);
        P.closing = true;
        for (auto& dv : P.streams) {
            for (auto it = dv.second.begin(); it != dv.second.end();) {
                if (!P.dedicated.erase(it->second)) { ++it; continue; }
                gone.push_back(it->second);
                P.stream_index.erase(it->second);
                P.dedicated_made[dv.first]--;
                it = dv.second.erase(it);
            }
        }
    }
    for (hipStream_t s : gone) if (hipStreamDestroy(s) != hipSuccess) (void)hipGetLastError();      // (waits for the stream's work)
}
// 0: a stream; -1: the runtime failed; -2: no stream left within the queue budget (the caller shares one it has)
inline int stream_create(Stream* s) {
    Pools& P = Pools::get();
    const int dev = current_device();
    const QueueBudget qb = queue_budget(dev);           // (takes its own lock; hipFuncGetAttributes on first use)
    std::lock_guard<std::mutex> g(P.mu);
    auto& v = P.streams[dev];
    if (!v.empty()) { *s = v.begin()->second; v.erase(v.begin()); return 0; }
    // Dedicated hardware queues: the runtime gives a stream created with a compute-unit mask (here: all ones, no restriction)
    // a hardware queue of its own instead of a share of the GPU_MAX_HW_QUEUES pool.  For a process whose first HIP call came
    // BEFORE this library was loaded (any torch user) the pool is fixed at the runtime's default of 4, several jobs share a
    // queue and a long narrow kernel blocks the others (1.30 M proof_verify/s instead of 1.50 M; with dedicated queues 1.50 M
    // whatever the pool, profiles/r04_f_dedicated_queues.log; on the present library profiles/auto_queues_ab.log).  How many:
    // queue_policy.hpp -- bbs_runtime_set_dedicated_queues / BBS_DEDICATED_QUEUES=k asks for k, 0 switches them off, and with
    // nothing set the library makes up what the effective pool (load_state above) lacks of its own 20; always within the
    // scratch budget, counted in queues actually touched.  Such streams are BLOCKING with respect to the legacy default stream
    // (the runtime offers no flags for them): a host that runs its own kernels on stream 0 beside the jobs sets 0.
    const int setting = dedicated_setting();
    qpolicy::Kind kind = qpolicy::next_stream(effective_pool(), qb.pool, qb.total, setting, P.dedicated_made[dev], P.pooled_made[dev]);
    if (kind == qpolicy::DEDICATED) {
        uint32_t mask[16];
        for (auto& m : mask) m = 0xFFFFFFFFu;
        if (hipExtStreamCreateWithCUMask(s, 16, mask) == hipSuccess) {
            P.dedicated_made[dev]++;
            P.dedicated.insert(*s);
            static std::once_flag at_exit;
            std::call_once(at_exit, []() { (void)std::atexit(release_dedicated_streams_at_exit); });
        } else {                                           // the runtime has none to give: as if none had been wished for
            (void)hipGetLastError();
            kind = qpolicy::next_stream(effective_pool(), qb.pool, qb.total, 0, P.dedicated_made[dev], P.pooled_made[dev]);
        }
    }
    // the pool alone may be over budget (an explicit GPU_MAX_HW_QUEUES): streams map onto its queues round robin, so the number
    // of pooled streams this library creates bounds the number of pooled queues it touches
    if (kind == qpolicy::NONE) return -2;
    if (kind == qpolicy::POOLED) {
        if (hipStreamCreateWithFlags(s, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); return -1; }
        P.pooled_made[dev]++;
    }
    P.stream_index[*s] = P.next_stream_index++;
    return 0;
}
// streams of the device made so far and not destroyed (alive or recycled here), by kind
inline void queue_counts(int dev, int* dedicated, int* pooled) {
    Pools& P = Pools::get();
    std::lock_guard<std::mutex> g(P.mu);
    *dedicated = P.dedicated_made[dev];
    *pooled = P.pooled_made[dev];
}
inline void stream_destroy(Stream& s) {                  // callers synchronise the stream first
    Pools& P = Pools::get();
    std::lock_guard<std::mutex> g(P.mu);
    auto& v = P.streams[current_device()];
    auto it = P.stream_index.find(s);
    if (it != P.stream_index.end() && v.size() < 256 && !(P.closing && P.dedicated.count(s))) { v.insert({it->second, s}); return; }
    if (it != P.stream_index.end()) P.stream_index.erase(it);
    if (P.dedicated.erase(s)) P.dedicated_made[current_device()]--; else P.pooled_made[current_device()]--;
    (void)hipStreamDestroy(s);
}
inline int event_create(Event* e) {
    {
        Pools& P = Pools::get();
        std::lock_guard<std::mutex> g(P.mu);
        auto& v = P.events[current_device()];
        if (!v.empty()) { *e = v.back(); v.pop_back(); return 0; }
    }
    return hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess ? 0 : -1;
}
inline void event_destroy(Event& e) {
    Pools& P = Pools::get();
    std::lock_guard<std::mutex> g(P.mu);
    auto& v = P.events[current_device()];
    if (v.size() < 512) v.push_back(e); else (void)hipEventDestroy(e);
}
inline int event_record(Event& e, Stream& s) { return hipEventRecord(e, s) == hipSuccess ? 0 : -1; }
inline int stream_wait(Stream& s, Event& e) { return hipStreamWaitEvent(s, e, 0) == hipSuccess ? 0 : -1; }
// everything in front of the event's last record has finished (an event never recorded counts as done)
inline bool event_done(Event& e) {
    if (hipEventQuery(e) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
}

// stages may declare `static constexpr int WAVES_PER_EU = k;` to cap their register allocation at
// 512 / k VGPRs so that k wavefronts fit on one SIMD
template <class F, class = void> struct waves_of { static constexpr int v = 1; };
template <class F> struct waves_of<F, std::void_t<decltype(F::WAVES_PER_EU)>> { static constexpr int v = F::WAVES_PER_EU; };

template <class F, class A>
__global__ void __launch_bounds__(64, waves_of<F>::v) k_stage(A a, size_t nthreads) {
    const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (t < nthreads) F::run(a, t);
}
// every kernel of the library is known when the library has been loaded (queue budget above)
template <class F, class A> struct KernelEntry { static const int token; };
template <class F, class A> const int KernelEntry<F, A>::token = register_kernel(reinterpret_cast<const void*>(&k_stage<F, A>));
template <class F, class A>
inline int launch(Stream& s, const A& a, size_t nthreads) {
    if (!nthreads) return 0;
    (void)&KernelEntry<F, A>::token;
    const unsigned blocks = (unsigned)((nthreads + 63) / 64);
    hipLaunchKernelGGL((k_stage<F, A>), dim3(blocks), dim3(64), 0, s, a, nthreads);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// HIP events recorded on the stream the kernels are launched on; read back after ONE
// synchronisation so that timing does not serialise host and device between stages
struct EventList {
    std::vector<hipEvent_t> ev;
    size_t used = 0;
    int dev = 0;
    explicit EventList(size_t cap) : ev(cap, nullptr), dev(current_device()) {
        Pools& P = Pools::get();
        std::lock_guard<std::mutex> g(P.mu);
        auto& v = P.timing_events[dev];
        for (auto& e : ev) {
            if (!v.empty()) { e = v.back(); v.pop_back(); }
            else (void)hipEventCreate(&e);
        }
    }
    ~EventList() {
        Pools& P = Pools::get();
        std::lock_guard<std::mutex> g(P.mu);
        auto& v = P.timing_events[dev];
        for (auto& e : ev) if (e) { if (v.size() < 4096) v.push_back(e); else (void)hipEventDestroy(e); }
    }
    int record(Stream& s) { return (used < ev.size() && hipEventRecord(ev[used++], s) == hipSuccess) ? 0 : -1; }
    int finish(Stream& s) { return hipStreamSynchronize(s) == hipSuccess ? 0 : -1; }
    float ms(size_t a, size_t b) { float m = 0; (void)hipEventElapsedTime(&m, ev[a], ev[b]); return m; }
};
#endif
}  // namespace rt

// device buffer with ownership
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    int dev = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() { if (p) rt::dfree(p, bytes, dev); p = nullptr; bytes = 0; }
    int alloc(size_t b) { release(); bytes = b; dev = rt::current_device(); if (rt::dmalloc(&p, b)) { p = nullptr; bytes = 0; return -1; } return 0; }
    void swap(DevBuf& o) { std::swap(p, o.p); std::swap(bytes, o.bytes); std::swap(dev, o.dev); }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// page-locked host staging buffer with ownership
struct HostBuf {
    void* p = nullptr;
    size_t bytes = 0;
    HostBuf() = default;
    HostBuf(const HostBuf&) = delete;
    HostBuf& operator=(const HostBuf&) = delete;
    ~HostBuf() { release(); }
    void release() { if (p) rt::hfree(p, bytes); p = nullptr; bytes = 0; }
    int alloc(size_t b) { release(); bytes = b; return rt::hmalloc(&p, b); }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// no internal state (stages.hpp ST_PENDING / ST_PAIRING) may leave the library: an item still in one was never decided
inline bool statuses_final(const int8_t* st, size_t n) {
    for (size_t i = 0; i < n; i++) if (st[i] == ST_PENDING || st[i] == ST_PAIRING) return false;
    return true;
}

// =============================================================================================
// host-side packing helpers
// =============================================================================================
inline uint32_t le32(const uint8_t* b) {
    return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
}
inline void put_le32(uint8_t* b, uint32_t v) {
    b[0] = (uint8_t)v; b[1] = (uint8_t)(v >> 8); b[2] = (uint8_t)(v >> 16); b[3] = (uint8_t)(v >> 24);
}

// SoA array of `words` 32-bit words per item.  Filled item by item into an item-major staging area (the writes of
// one item are contiguous; writing word-major directly strides by n words and misses the cache on every store), then
// transposed in 16-item tiles into the word-major layout the kernels read: soa().
struct Soa {
    std::vector<uint32_t> aos, v;
    size_t n = 0, words = 0;
    bool sealed = false;
    void init(size_t words_, size_t n_) { words = words_; n = n_; aos.assign(words_ * n_, 0u); v.clear(); sealed = false; }
    uint32_t& at(size_t w, size_t i) { return aos[i * words + w]; }
    size_t bytes() const { return aos.size() * 4; }
    const std::vector<uint32_t>& soa() {
        if (!sealed) {
            v.resize(aos.size());
            constexpr size_t T = 16;
            for (size_t i0 = 0; i0 < n; i0 += T) {
                const size_t m = std::min(T, n - i0);
                for (size_t w = 0; w < words; w++) {
                    uint32_t* dst = v.data() + w * n + i0;
                    const uint32_t* src = aos.data() + i0 * words + w;
                    for (size_t k = 0; k < m; k++) dst[k] = src[k * words];
                }
            }
            sealed = true;
        }
        return v;
    }
};

// canonical scalar (32 B LE) into SoA words [w0, w0+8); returns false if >= r
template <class P>
inline bool pack_fe(Soa& s, size_t w0, size_t i, const uint8_t* le) {
    uint32_t l[P::NC];
    for (int k = 0; k < P::NC; k++) l[k] = le32(le + 4 * k);
    for (int k = 0; k < P::NC; k++) s.at(w0 + k, i) = l[k];
    return limbs_lt_mod<P>(l);
}
template <class C>
inline bool pack_g1(Soa& s, size_t w0, size_t i, const uint8_t* xy) {
    constexpr int NC = C::FpP::NC;
    bool a = pack_fe<typename C::FpP>(s, w0, i, xy);
    bool b = pack_fe<typename C::FpP>(s, w0 + NC, i, xy + 4 * NC);
    return a && b;
}
inline void unpack_words_le(const uint32_t* v, size_t n, size_t w0, size_t i, int words, uint8_t* out) {
    for (int k = 0; k < words; k++) put_le32(out + 4 * k, v[(w0 + k) * n + i]);
}
inline void unpack_words_le(const std::vector<uint32_t>& v, size_t n, size_t w0, size_t i, int words, uint8_t* out) {
    unpack_words_le(v.data(), n, w0, i, words, out);
}

// ragged bytes -> device pool + u32 offset / len
struct BytePool {
    std::vector<uint8_t> bytes;
    std::vector<uint32_t> off, len;
    bool build(size_t n, const uint8_t* data, const uint64_t* offs) {
        off.assign(n, 0); len.assign(n, 0);
        if (!offs) { bytes.assign(4, 0); return true; }        // all empty
        const uint64_t total = offs[n] - offs[0];
        if (total > 0xF0000000ull) return false;
        for (size_t i = 0; i < n; i++) {
            if (offs[i + 1] < offs[i]) return false;
            off[i] = (uint32_t)(offs[i] - offs[0]);
            len[i] = (uint32_t)(offs[i + 1] - offs[i]);
        }
        bytes.assign(data ? data + offs[0] : nullptr, data ? data + offs[n] : nullptr);
        if (bytes.size() != total) return false;
        bytes.resize(bytes.size() + 4, 0);
        return true;
    }
};

// =============================================================================================
// context
// =============================================================================================
// jobs alive per DEVICE, whatever context they belong to: what the AUTO form of a job goes by (Ctx::latency_form_now).
// A process that drives one GPU through several contexts -- an issuer with one context per message count, a BLS12-381 and
// a BN254 engine side by side (mixed.py) -- shares the chip among all their jobs; counting per context would give every
// one of them the latency form (more instructions for a shorter path) exactly where throughput decides.
inline std::atomic<int>& device_live_jobs(int dev) {
    static std::atomic<int> live[64];
    return live[(unsigned)dev & 63u];
}
struct IJob;
struct bbs_ctx {
    int curve = 0;
    bool stage_timing = false;       // jobs created from now on record HIP events around every stage of every run
    virtual ~bbs_ctx() {}
};

template <class C>
struct Ctx : bbs_ctx {
    static constexpr int N = C::FpP::N;          // internal limbs
    static constexpr int FPB = 4 * C::FpP::NC;   // bytes of a canonical field element
    int device = 0;
    rt::Stream stream{};
    bool stream_ready = false;
    int win_bits = 8;                // width of the tables that are built
    int win_bits_requested = 0;      // bbs_ctx_set_window_bits; 0 (the default) = choose at set_generators from the free device memory
    // host state
    bool gens_set = false, pk_set = false, sk_set = false, dst_too_long = false;
    int L = 0;
    std::vector<G1Aff<C>> gens;      // Q1, H_1..H_L  (Montgomery)
    std::vector<uint8_t> api_id;
    G2Aff<C> pk{};
    uint32_t sk[8] = {0};
    // device state
    CtxConsts<C> hc{};               // host mirror
    DevBuf d_consts, d_tables, d_winbase, d_bases;
    bool consts_dirty = true;
    // key set of the keyed entry points (bbs_ctx_set_public_keys, keyed.hpp): immutable once built; a keyed job holds a
    // reference, so replacing the set never changes a job in flight, and the device array goes with its last holder
    struct KeySet {
        size_t n = 0;
        std::vector<int8_t> status;  // per key: 1 accepted, BBS_ST_NOT_ON_CURVE refused
        std::vector<G2Aff<C>> pk;    // host copy of every key (a refused key: the identity, never read): what its prefixes per length are hashed from
        DevBuf d;                    // [n] KeyEntry<C>
        bool unit = false;           // form of every line table of the set (lines_unit() when it was built)
        uint64_t lineage = 0;        // the same for a set and every set appended to it, new for a set that replaces one (SignSet)
    };
    std::shared_ptr<const KeySet> keys;
    // Signing key set of keyed sign (bbs_ctx_set_secret_keys / bbs_ctx_add_secret_keys, op_kg.hpp): the secret halves of the key
    // set, row k = the 8 canonical words of sk_k whose public half sk_k * BP2 is key k of `keys`.  The rules of KeySet --
    // immutable once built, grows by appending (a new array of exactly n_old + n rows, the old rows copied device to device), a
    // keyed sign job holds a reference -- plus one: the device array is CLEARED before it is released, whoever lets go last (the
    // context, a job, a setter).  It keeps no host copy of a secret.  The set covers the keys [0, n) of the key set it was built
    // beside (same lineage); a key appended public-only lies beyond n or has has[k] == 0 and a zero row, as a refused key has.
    struct SignSet {
        size_t n = 0, n_secret = 0;  // rows; rows with a secret half
        uint64_t lineage = 0;        // of the key set the rows belong to
        std::vector<uint8_t> has;    // per row: 1 = key k has a secret half
        DevBuf d;                    // [n][8] words
        int device = 0;
        ~SignSet() {                 // cleared and synchronised, only then back to the pool (a stream of its own: every holder has synchronised its streams)
            if (!d.p) return;
            (void)rt::set_device(device);
            rt::Stream s{};
            (void)rt::dmemset(d.p, 0, d.bytes, s);
            (void)rt::sync(s);
        }
    };
    std::shared_ptr<const SignSet> sign_keys;
    size_t secret_key_count() const { const auto ss = sign_keys; return ss ? ss->n_secret : 0; }
    void drop_key_sets() { keys.reset(); key_lens.reset(); sign_keys.reset(); }
    // keyed jobs of mixed message counts (bbs_ctx_set_keyed_mixed_lengths): off by default, independent of mixed_lengths below.
    // On: the keyed verify / proof_verify jobs created from now on accept item i under its own key k_i with its own count
    // l_i <= L.  The one datum that depends on both is the domain prefix: one HashCtx per (key, length), row k of KeyLenSet =
    // what rebuild_hash builds per length for the context's own key.  Built EAGERLY on host threads -- by the setter for the
    // keys that exist, by add_keys for the keys it appends (the old rows are copied device to device) -- so while the switch is
    // on key_lens always belongs to `keys`.  Immutable once built; a job holds a reference (JobBase::key_len_set).  The rows of a
    // refused key hold key_hash0() and are never read: KeyGate decides such an item before the scalar stage looks at it.
    bool keyed_mixed_lengths = false;
    struct KeyLenSet {
        std::shared_ptr<const KeySet> of;        // the key set these rows were built for
        size_t stride = 0;                       // L + 1
        DevBuf d;                                // [of->n][stride] HashCtx
    };
    std::shared_ptr<const KeyLenSet> key_lens;
    size_t key_lens_bytes() const { const auto kl = key_lens; return keyed_mixed_lengths && kl ? kl->of->n * kl->stride * sizeof(HashCtx) : 0; }
    // Job-local key sets (bbs_*_with_keys_*, op_key.hpp job_keys_prepare): what KeyBuild and KeyLenBuild read beside the keys,
    // the same for every key and every job of the context: key_hash0() || I2OSP(L, 8) || compressed_gens() || api_id.  Uploaded
    // when the first such job is created, dropped by set_generators; a job holds a reference.  Never built where the exports
    // are not used.
    struct KeyBlob {
        DevBuf d;
        size_t api_len = 0, gens_bytes = 0;
        const HashCtx* hash0() const { return d.as<HashCtx>(); }
        const uint8_t* suffix() const { return d.as<uint8_t>() + sizeof(HashCtx); }       // I2OSP(L, 8) || gens || api_id
        size_t suffix_len() const { return 8 + gens_bytes + api_len; }
        const uint8_t* cg() const { return suffix() + 8; }
        const uint8_t* api() const { return cg() + gens_bytes; }
    };
    std::shared_ptr<const KeyBlob> key_blob;
    int sync_key_blob(std::shared_ptr<const KeyBlob>& out) {
        std::lock_guard<std::mutex> g(mu);
        if (!gens_set) return BBS_E_STATE;
        if (!key_blob) {
            std::vector<uint8_t> blob(sizeof(HashCtx));
            const HashCtx h0 = key_hash0();
            std::memcpy(blob.data(), &h0, sizeof(h0));
            for (int k = 7; k >= 0; k--) blob.push_back((uint8_t)((uint64_t)L >> (8 * k)));
            const std::vector<uint8_t> cg = compressed_gens();
            blob.insert(blob.end(), cg.begin(), cg.end());
            blob.insert(blob.end(), api_id.begin(), api_id.end());
            std::shared_ptr<KeyBlob> kb(new KeyBlob());
            kb->api_len = api_id.size(); kb->gens_bytes = cg.size();
            if (kb->d.alloc(blob.size())) return BBS_E_NOMEM;
            if (rt::h2d(kb->d.p, blob.data(), blob.size(), stream) || rt::sync(stream)) return BBS_E_HIP;
            key_blob = std::move(kb);
        }
        out = key_blob;
        return BBS_OK;
    }
    // The job-local key cache (bbs_ctx_set_job_key_cache; job_form.hpp job_keys_begin, DESIGN.md 8 "Job-local key cache"): off by
    // default (capacity 0).  On: the prepared keys of the bbs_*_with_keys_* jobs stay in `capacity` slots on the device, found
    // again by their whole compressed string (key_cache.hpp).  ONE generation = the entries prepared under one KeyBlob (generators,
    // api_id), one line form and one row stride (0, or L + 1 under keyed mixed lengths); a job whose form differs starts a new,
    // empty generation, the old one lives on through the jobs that hold it.  The device arrays are allocated by the first cached
    // job of a generation.  Everything here is read and written under `mu`.
    struct KeyCacheEvent {               // behind the publishing kernel of one job; its slots carry it until it has completed
        rt::Event ev{};
        int device = 0;
        bool ok = false;
        ~KeyCacheEvent() { if (ok) { (void)rt::set_device(device); rt::event_destroy(ev); } }
    };
    struct KeyCacheGen {
        KeyCacheBook book;
        std::shared_ptr<const KeyBlob> blob;
        bool unit = false;
        uint32_t stride = 0;
        DevBuf entries, status, rows;    // [capacity] KeyEntry<C>, [capacity] codes, [capacity][stride] HashCtx
        std::vector<std::shared_ptr<KeyCacheEvent>> slot_event;      // null: nothing to wait for
        KeyCacheGen(size_t cap, size_t key_bytes) : book(cap, key_bytes), slot_event(cap) {}
        size_t device_bytes() const { return entries.bytes + status.bytes + rows.bytes; }
    };
    size_t job_key_cache_cap = 0;
    std::shared_ptr<KeyCacheGen> job_key_cache;
    KeyCacheCounters job_key_cache_counters;
    int set_job_key_cache(size_t capacity_keys) {
        if (capacity_keys > 0xFFFFFFF0ull) return BBS_E_ARG;
        std::lock_guard<std::mutex> g(mu);
        if (capacity_keys != job_key_cache_cap) job_key_cache.reset();
        job_key_cache_cap = capacity_keys;
        return BBS_OK;
    }
    void job_key_cache_report(size_t* capacity, size_t* resident, size_t* pinned, uint64_t* hits, uint64_t* misses, uint64_t* evictions,
                              uint64_t* bypassed_jobs, size_t* device_bytes) {
        std::lock_guard<std::mutex> g(mu);
        const auto gen = job_key_cache;
        const KeyCacheCounters& c = job_key_cache_counters;
        if (capacity) *capacity = job_key_cache_cap;
        if (resident) *resident = gen ? gen->book.resident() : 0;
        if (pinned) *pinned = gen ? gen->book.pinned() : 0;
        if (hits) *hits = c.hits;
        if (misses) *misses = c.misses;
        if (evictions) *evictions = c.evictions;
        if (bypassed_jobs) *bypassed_jobs = c.bypassed_jobs;
        if (device_bytes) *device_bytes = gen ? gen->device_bytes() : 0;
    }
    // The generation a job of this form uses (mu is held): the current one if it was built under the same blob, line form and
    // stride, else a new, empty one in its place.  The arrays are allocated here, by the first job that needs them.
    int job_key_cache_gen(const std::shared_ptr<const KeyBlob>& kb, bool unit, uint32_t stride, std::shared_ptr<KeyCacheGen>& out) {
        auto gen = job_key_cache;
        if (!gen || gen->blob != kb || gen->unit != unit || gen->stride != stride) {
            gen.reset(new KeyCacheGen(job_key_cache_cap, 2 * (size_t)FPB));
            gen->blob = kb; gen->unit = unit; gen->stride = stride;
            const size_t cap = job_key_cache_cap;
            if (gen->entries.alloc(cap * sizeof(KeyEntry<C>)) || gen->status.alloc(cap) || (stride && gen->rows.alloc(cap * stride * sizeof(HashCtx)))) return BBS_E_NOMEM;
            job_key_cache = gen;
        }
        out = gen;
        return BBS_OK;
    }
    // mixed message counts (bbs_ctx_set_mixed_lengths): off by default.  On: the single-key verify / proof_verify jobs created
    // from now on accept item i with its own count l_i <= L; the only data of a context that depend on the count are the domain
    // prefixes, one HashCtx per length 0 .. L (prefix l = the first l + 1 generators: create_generators is prefix-consistent).
    // The host mirror is rebuilt by rebuild_hash like hc.hash and uploaded by sync_lengths when the next job is created; the
    // device array is immutable once built and a job holds a reference, so a change of key or generators never reaches a job
    // that exists (the rule of the key set above).
    bool mixed_lengths = false;
    // the same for the producing side (bbs_ctx_set_mixed_lengths_gen): off by default and independent of mixed_lengths.  On: the
    // sign / proof_gen jobs created from now on accept item i with its own count l_i <= L.  Both switches are served by the ONE
    // array of prefixes below -- built while either is on, counted once by table_bytes.  (A context that signs has its public
    // key: set_secret_key derives sk * BP2 and goes through set_pk_internal, so rebuild_hash sees pk_set on the signing side too.)
    bool mixed_lengths_gen = false;
    bool any_mixed_lengths() const { return mixed_lengths || mixed_lengths_gen; }
    // bbs_ctx_set_seeded_random_scalars: proof_gen jobs created while it is on read random_scalars / rnd_off as seeds and draw
    // on the device (stages_draw.hpp PgDraw) under this DST, kept as given (more than 255 bytes: every draw is refused)
    bool seeded_rnd = false;
    std::vector<uint8_t> seeded_dst;
    struct LenSet { DevBuf d; };     // [L + 1] HashCtx
    std::vector<HashCtx> len_hash;   // host mirror; empty unless one of the two switches is on and generators and key are set
    std::shared_ptr<const LenSet> len_set;      // null: to be uploaded from len_hash
    // batch verification (pippenger.hpp): off by default = every item gets its own pairing product
    bool batch_verify = false;
    // caller vouches that every G1 input is in the prime-order subgroup: variable-base multiplications of the
    // verification paths use the GLV split where the curve has it (g1.hpp); off by default
    bool points_in_subgroup = false;
    // latency form of a job (bbs_ctx_set_latency_mode): proof_verify's T1 as three multiplications on three lanes instead
    // of one joint chain, the two Miller loops of a pairing product on separate lane groups -- a shorter critical path for
    // more work.  0 = never, 1 = always, 2 = AUTO (default): a job gets the latency form iff at most one other job of
    // the DEVICE (any context, device_live_jobs) is alive when it is created, i.e. when it will have (most of) the chip to itself
    int latency_mode = 2;
    std::atomic<int> live_jobs{0};
    bool latency_form_now() const { return latency_mode == 1 || (latency_mode == 2 && device_live_jobs(device).load() <= 2); }
    bool fix_tree = false;           // bbs_ctx_set_fixed_base_tree: the fixed-base sums as trees of affine additions
    // Form of the Miller-loop line tables (pairing.hpp "Unit form", bbs_ctx_set_unit_lines).  ONE form per context: BP2's table,
    // the public key's and every table of the key set have it, so a pairing kernel holds one form and a job picks its kernel
    // by it -- for a keyed job that is the AND over its key set.  unit_lines is what the caller asked for (default: unit); a
    // key whose walk meets c = 0 has no unit form, and while the context holds such a key every table is kept in the
    // (c, nl) form (rebuild_lines, op_key.hpp).  dev_lines_unit is the form of the constants on the DEVICE (sync_consts),
    // which is what a launch goes by.  Like a change of key, a change of form is for a context without jobs in flight.
    bool unit_lines = true;
    bool dev_lines_unit = false;
    bool lines_unit() const { return hc.tab_bp2.unit != 0; }
    bool lines_form_stale() const {  // a table in the other form, or the unit form wanted and not held
        return (!hc.tab_pk.q_is_identity && hc.tab_pk.unit != hc.tab_bp2.unit) || (unit_lines && !lines_unit());
    }
    int rebuild_lines();             // every table again: the form asked for, or (c, nl) where some key has no unit form
    int set_unit_lines(int enabled) {
        std::lock_guard<std::mutex> g(mu);
        unit_lines = enabled != 0;
        if (lines_unit() == unit_lines) return BBS_OK;
        return rebuild_lines();
    }
    uint32_t rlc_seed[8] = {0};
    uint64_t rlc_counter = 0;
    std::mutex mu;                   // uploads may come from several host threads: counter and constant sync

    // secret seed of the next batch: SHA-256(context seed || counter)
    void next_rlc_seed(uint32_t* out8) {
        std::lock_guard<std::mutex> g(mu);
        Sha256 s;
        sha256_init(s);
        for (int k = 0; k < 8; k++) sha256_word(s, rlc_seed[k]);
        sha256_u64be(s, rlc_counter++);
        sha256_final(s, out8);
    }
    // the context's secret seed: the caller's 32 bytes, or (NULL) the operating system's
    int set_rlc_seed(const uint8_t* seed32) {
        uint8_t buf[32];
        if (seed32) std::memcpy(buf, seed32, 32);
        else {
            FILE* f = std::fopen("/dev/urandom", "rb");
            const size_t got = f ? std::fread(buf, 1, 32, f) : 0;
            if (f) std::fclose(f);
            if (got != 32) return BBS_E_STATE;
        }
        for (int k = 0; k < 8; k++) rlc_seed[k] = le32(buf + 4 * k);
        rlc_counter = 0;
        return BBS_OK;
    }
    int set_batch_verification(int enabled, const uint8_t* seed32) {
        if (enabled) {
            if (const int rc = set_rlc_seed(seed32)) return rc;
        }
        batch_verify = enabled != 0;
        return BBS_OK;
    }
    // keyed batch verification (bbs_ctx_set_keyed_batch_verification; pippenger.hpp, job_form.hpp keyed_bv_plan): off by
    // default, independent of batch_verify -- single-key jobs never look at it, keyed jobs never look at batch_verify.  A
    // key forms a group in a job iff at least keyed_bv_min of the job's items name it.  The seed is the context's ONE seed
    // (next_rlc_seed): enabling either switch sets it and restarts the counter.
    // KEYED_BV_MIN_DEFAULT: measured (tools/keyed_bv_bench.py, profiles/keyed_bv_bench.json; DESIGN.md 8 has the table).  On the
    // 4096-item loop the combination LOSES at 64 and at 128 items per key (the bucket kernel spends a 256-bucket suffix sum on
    // every segment, however short) and wins for proof_verify at 256 items per key, the smallest size measured at which it
    // does; verify is even there and wins at 4096.  Never below 17 -- a group of 16 or fewer items costs more pairing products
    // combined than alone.
    static constexpr size_t KEYED_BV_MIN_DEFAULT = 256;
    bool keyed_bv = false;
    size_t keyed_bv_min = KEYED_BV_MIN_DEFAULT;
    int set_keyed_batch_verification(int enabled, const uint8_t* seed32, size_t min_items_per_key) {
        if (enabled) {
            if (const int rc = set_rlc_seed(seed32)) return rc;
            keyed_bv_min = min_items_per_key ? min_items_per_key : KEYED_BV_MIN_DEFAULT;
        }
        keyed_bv = enabled != 0;
        return BBS_OK;
    }

    int init(int dev) {
        device = dev;
        if (rt::set_device(dev)) return BBS_E_NO_DEVICE;
        if (const int src = rt::stream_create(&stream)) return src == -2 ? BBS_E_NO_RESOURCES : BBS_E_HIP;
        stream_ready = true;
        std::memset(&hc, 0, sizeof(hc));
        for (int j = 0; j < N; j++) { hc.p1.x.v[j] = C::K::P1X_M[j]; hc.p1.y.v[j] = C::K::P1Y_M[j]; }
        for (int k = 0; k < 3; k++) for (int m = 0; m < 6; m++) for (int c2 = 0; c2 < 2; c2++)
            for (int j = 0; j < N; j++) hc.frob[k][m][c2][j] = C::K::FROB[k][m][c2][j];
        build_schedule<C>(hc.sched);
        if (!build_line_table<C>(g2_generator<C>(), hc.tab_bp2, unit_lines)) return BBS_E_ARG;
        hc.tab_pk.q_is_identity = 1;
        hc.tab_pk.n_lines = 0;
        if (d_consts.alloc(sizeof(CtxConsts<C>))) return BBS_E_NOMEM;
        return BBS_OK;
    }
    ~Ctx() override {
        (void)rt::set_device(device);
        if (stream_ready) { (void)rt::sync(stream); rt::stream_destroy(stream); }
        volatile uint32_t* s = sk;                       // do not leave the secret key in freed host memory
        for (int k = 0; k < 8; k++) s[k] = 0;
    }

    int use() { return rt::set_device(device) ? BBS_E_HIP : BBS_OK; }
    size_t table_bytes() const {
        return d_tables.bytes + d_winbase.bytes + d_bases.bytes + d_consts.bytes + (any_mixed_lengths() ? len_hash.size() * sizeof(HashCtx) : 0) + key_lens_bytes() +
               seeded_dst.size();
    }

    // domain prefix:  Z_pad || compress(pk) || I2OSP(L,8) || compress(Q1) || compress(H_i).. || api_id
    void rebuild_hash() {
        HashCtx& h = hc.hash;
        std::memset(&h, 0, sizeof(h));
        std::vector<uint8_t> dst(api_id);
        const char* suf = "H2S_";
        dst.insert(dst.end(), suf, suf + 4);
        dst_too_long = dst.size() > 255;
        if (!dst_too_long) { std::memcpy(h.dst_h2s, dst.data(), dst.size()); h.dst_h2s_len = (uint32_t)dst.size(); }
        len_hash.clear();
        len_set.reset();
        if (!(gens_set && pk_set)) { consts_dirty = true; return; }
        domain_midstate(pk, h);
        if (any_mixed_lengths()) {
            // every generator is compressed ONCE; prefix l hashes the first l + 1 of them
            const std::vector<uint8_t> cg = compressed_gens();
            len_hash.assign((size_t)L + 1, key_hash0());
            for (int l = 0; l <= L; l++) domain_midstate(pk, len_hash[(size_t)l], l, cg.data());
        }
        consts_dirty = true;
    }
    std::vector<uint8_t> compressed_gens() const {      // compress(Q1) || compress(H_1) || .. || compress(H_L)
        std::vector<uint8_t> cg(gens.size() * FPB);
        for (size_t k = 0; k < gens.size(); k++) g1_compress_host<C>(gens[k], cg.data() + k * FPB);
        return cg;
    }
    // the key-dependent part of the domain prefix (needs the generators): dom_* of h for key q and the first l message
    // generators (l < 0: all L of them); cg: compressed_gens() of the caller, where it builds many prefixes
    void domain_midstate(const G2Aff<C>& q, HashCtx& h, int l = -1, const uint8_t* cg = nullptr) const {
        if (l < 0) l = L;
        Sha256 s;
        xmd48_begin(s);
        uint8_t buf[4 * FPB];
        g2_compress<C>(q, buf);
        sha256_bytes(s, buf, 2 * FPB);
        sha256_u64be(s, (uint64_t)l);
        if (cg) sha256_bytes(s, cg, (uint32_t)((size_t)(l + 1) * FPB));
        else for (int k = 0; k <= l; k++) { g1_compress_host<C>(gens[(size_t)k], buf); sha256_bytes(s, buf, FPB); }
        sha256_bytes(s, api_id.data(), (uint32_t)api_id.size());
        for (int k = 0; k < 8; k++) h.dom_mid[k] = s.h[k];
        h.dom_mid_total = s.total - s.fill;
        h.dom_tail_len = s.fill;
        for (uint32_t k = 0; k < s.fill; k++) h.dom_tail[k] = (uint8_t)(s.w[k >> 2] >> ((3 - (k & 3)) * 8));
    }

    int sync_consts() {
        std::lock_guard<std::mutex> g(mu);
        if (!consts_dirty) return BBS_OK;
        hc.tables = d_tables.as<uint32_t>();
        if (rt::h2d(d_consts.p, &hc, sizeof(hc), stream)) return BBS_E_HIP;
        dev_lines_unit = lines_unit();
        consts_dirty = false;
        return BBS_OK;
    }

    int set_mixed_lengths(int enabled) {
        std::lock_guard<std::mutex> g(mu);
        if (mixed_lengths == (enabled != 0)) return BBS_OK;
        mixed_lengths = enabled != 0;
        rebuild_hash();
        return BBS_OK;
    }
    int set_mixed_lengths_gen(int enabled) {
        std::lock_guard<std::mutex> g(mu);
        if (mixed_lengths_gen == (enabled != 0)) return BBS_OK;
        mixed_lengths_gen = enabled != 0;
        rebuild_hash();
        return BBS_OK;
    }
    // the per-length prefixes on the device, for a job that is being created (uploaded once per rebuild_hash)
    int sync_lengths(std::shared_ptr<const LenSet>& out) {
        std::lock_guard<std::mutex> g(mu);
        if (!any_mixed_lengths() || len_hash.empty()) return BBS_E_STATE;
        if (!len_set) {
            std::shared_ptr<LenSet> ls(new LenSet());
            const size_t b = len_hash.size() * sizeof(HashCtx);
            if (ls->d.alloc(b)) return BBS_E_NOMEM;
            if (rt::h2d(ls->d.p, len_hash.data(), b, stream)) return BBS_E_HIP;
            len_set = std::move(ls);
        }
        out = len_set;
        return BBS_OK;
    }

    int set_generators(const uint8_t* g, size_t count, const uint8_t* aid, size_t aid_len);   // op_prim.hpp

    int set_pk_internal(const G2Aff<C>& q) {
        if (!g2_on_curve<C>(q) || !g2_in_subgroup<C>(q)) return BBS_E_PUBLIC_KEY;
        if (!build_line_table<C>(q, hc.tab_pk, lines_unit())) return BBS_E_PUBLIC_KEY;
        pk = q;
        pk_set = true;
        if (lines_form_stale()) {
            if (const int rc = rebuild_lines()) return rc;
        }
        rebuild_hash();
        return BBS_OK;
    }
    int set_public_key(const uint8_t* b, int is_identity) {
        G2Aff<C> q{};
        q.inf = is_identity != 0;
        if (!q.inf) {
            if (!b) return BBS_E_ARG;
            using P = typename C::FpP;
            if (!fe_from_le_bytes<P>(b, q.x.c0) || !fe_from_le_bytes<P>(b + FPB, q.x.c1) ||
                !fe_from_le_bytes<P>(b + 2 * FPB, q.y.c0) || !fe_from_le_bytes<P>(b + 3 * FPB, q.y.c1))
                return BBS_E_PUBLIC_KEY;
        } else {
            q.x = f2_zero<C>(); q.y = f2_zero<C>();
        }
        sk_set = false;
        return set_pk_internal(q);
    }
    // Key registration (op_key.hpp; stages_key.hpp has the device stage).  A set grows by APPENDING: add_keys builds a new
    // immutable KeySet of n_old + n entries -- exactly that many, nothing is over-allocated -- copies the old entries device to
    // device on the context's stream, prepares the n new entries in place behind them and swaps the pointer; jobs in flight keep
    // the set they hold, a failure leaves the old set.  bbs_ctx_set_public_keys is "new empty set + add".  Needs the generators
    // (set_generators drops the set: its midstates would be stale).
    // Every call prepares its new keys on up to 16 host threads (host_key_entry), as every registration did before.  The device
    // stage KeyBuild (stages_key.hpp) computes the same entries, byte for byte, but it has NOT BEEN TIMED against the host
    // threads, so no call of the library uses it yet: it is reachable through bbs_selftest_key_entries (path 1) only.
    // tools/keyed_bench.py --reg-only times both; a threshold belongs here once that table exists (DESIGN.md 8 "Registration").
    static constexpr bool KEY_BUILD_ON_DEVICE = false;
    HashCtx key_hash0() const {      // what every entry's HashCtx starts from: dst_h2s of the context, dom_* zero
        HashCtx h;
        std::memset(&h, 0, sizeof(h));
        std::memcpy(h.dst_h2s, hc.hash.dst_h2s, sizeof(h.dst_h2s));
        h.dst_h2s_len = hc.hash.dst_h2s_len;
        return h;
    }
    int8_t host_key_entry(const uint8_t* rec, bool is_inf, const uint8_t* oct, KeyEntry<C>& e, uint8_t* rec_out, int8_t* inf_out,
                          G2Aff<C>* q_out = nullptr) const;
    int key_build(KeyEntry<C>* d_out, size_t n, const uint8_t* rec, const int8_t* is_inf, const uint8_t* oct, bool on_device,
                  int8_t* status, uint8_t* rec_out, int8_t* inf_out, G2Aff<C>* q_out = nullptr, size_t* n_other_form = nullptr);
    // the prefixes per (key, length) of bbs_ctx_set_keyed_mixed_lengths (op_key.hpp)
    int build_key_lens(const std::shared_ptr<const KeySet>& ks, const std::shared_ptr<const KeyLenSet>& old, size_t n_old,
                       std::shared_ptr<const KeyLenSet>& out);
    int set_keyed_mixed_lengths(int enabled);
    int add_keys(bool replace, size_t n, const uint8_t* rec, const int8_t* is_inf, const uint8_t* oct, int8_t* key_status,
                 uint8_t* rec_out, int8_t* inf_out, uint32_t* first_index);
    int set_public_keys(size_t n_keys, const uint8_t* b, const int8_t* is_identity, int8_t* key_status) {
        if (n_keys && !b) return BBS_E_ARG;
        if (!n_keys) { drop_key_sets(); return BBS_OK; }
        const int rc = add_keys(true, n_keys, b, is_identity, nullptr, key_status, nullptr, nullptr, nullptr);
        if (!rc) sign_keys.reset();  // the new set has no secret halves (a failure leaves both sets)
        return rc;
    }
    size_t public_key_count() const { const auto ks = keys; return ks ? ks->n : 0; }
    int set_secret_key(const uint8_t* sk32) {
        if (!sk32) return BBS_E_ARG;
        uint32_t l[8];
        for (int k = 0; k < 8; k++) l[k] = le32(sk32 + 4 * k);
        if (!limbs_lt_mod<typename C::FrP>(l)) return BBS_E_ARG;
        std::memcpy(sk, l, sizeof(sk));
        int rc = set_pk_internal(g2_mul<C>(g2_generator<C>(), l));     // key_gen.rs:83-90
        if (rc) return rc;
        sk_set = true;
        return BBS_OK;
    }
    int get_public_key(uint8_t* out, int* inf) {
        if (!pk_set) return BBS_E_STATE;
        using P = typename C::FpP;
        if (inf) *inf = pk.inf ? 1 : 0;
        if (out) {
            if (pk.inf) std::memset(out, 0, 4 * FPB);
            else {
                fe_to_le_bytes<P>(pk.x.c0, out); fe_to_le_bytes<P>(pk.x.c1, out + FPB);
                fe_to_le_bytes<P>(pk.y.c0, out + 2 * FPB); fe_to_le_bytes<P>(pk.y.c1, out + 3 * FPB);
            }
        }
        return BBS_OK;
    }
};

// =============================================================================================
// jobs
// =============================================================================================
// Completion order (bbs_jobs_wait_any / bbs_job_poll).  Behind everything a run enqueues on a job's main stream the
// runtime places ONE host function (hipLaunchHostFunc); it stamps the job with the next sequence number and wakes the
// waiters -- the host thread sleeps on a condition variable, nothing polls the device.  A job may be armed more than once
// per run (the submit forms add their copies to page-locked memory behind run()): it is complete when every armed
// notification has fired.  The job's destructor synchronises its streams, so a notification never outlives its job.
struct CompletionHub {
    std::mutex mu;
    std::condition_variable cv;
    uint64_t seq = 0;
    static CompletionHub& get() { static CompletionHub* h = new CompletionHub(); return *h; }      // lives as long as the process
};
struct bbs_job {
    size_t n = 0;
    virtual ~bbs_job() {}
    std::atomic<uint32_t> armed{0};              // notifications placed behind this job's work (by its submitting thread)
    std::atomic<uint32_t> fired{0};
    std::atomic<uint64_t> done_seq{0};           // position in the process-wide completion order (of the last notification)
    static void on_complete(void* p) {
        bbs_job* j = static_cast<bbs_job*>(p);
        CompletionHub& h = CompletionHub::get();
        std::lock_guard<std::mutex> g(h.mu);
        j->done_seq.store(++h.seq, std::memory_order_relaxed);
        j->fired.fetch_add(1, std::memory_order_release);
        h.cv.notify_all();
    }
    // A run that could not be enqueued completely (a launch failed, the notification could not be placed): the job counts as
    // FINISHED WITH AN ERROR -- bbs_job_poll says 1, bbs_jobs_wait_any hands it out at once, and bbs_job_wait / wait_any
    // return BBS_E_HIP for it instead of delivering anything.  Without this a notification that was counted but never placed
    // left the job "running" for ever (wait_any slept on it), and a re-run that failed before arming left the PREVIOUS run's
    // completion standing, i.e. stale results reported as this run's.  Cleared when the next run starts.
    std::atomic<bool> failed{false};
    void mark_failed(bool take_back_arm) {
        CompletionHub& h = CompletionHub::get();
        std::lock_guard<std::mutex> g(h.mu);
        if (take_back_arm) armed.fetch_sub(1, std::memory_order_relaxed);
        failed.store(true, std::memory_order_release);
        h.cv.notify_all();
    }
    // behind what has been enqueued on the main stream so far (the main stream joins the side streams before its last stage).
    // Counted BEFORE the host function is placed (it may fire before hipLaunchHostFunc returns: counting afterwards could lose
    // the wake-up); taken back if it could not be placed.
    int arm_completion() {
        armed.fetch_add(1, std::memory_order_relaxed);
#ifdef BBS_HOST_TWIN
        on_complete(this);
        return BBS_OK;
#else
        if (!use() && hipLaunchHostFunc(stream(), &bbs_job::on_complete, this) == hipSuccess) return BBS_OK;
        (void)hipGetLastError();
        mark_failed(true);
        return BBS_E_HIP;
#endif
    }
    bool hold_arm = false;                       // the submit functions arm once, behind their own copies (not run())
    bool ever_run() const { return armed.load(std::memory_order_relaxed) != 0 || failed.load(std::memory_order_acquire); }
    bool completed() const {
        if (failed.load(std::memory_order_acquire)) return true;
        const uint32_t a = armed.load(std::memory_order_relaxed);
        return a != 0 && fired.load(std::memory_order_acquire) == a;
    }
    // aux = k > 0: the stage runs on the job's k-th side stream (k = 1, 2), concurrently with the main-stream stages
    // that follow the fork point (the place of the first stage of that stream in the list); join: bit k - 1 set = the main
    // stream first waits for everything issued on side stream k (1: the first, 2: the second, 3: both)
    static constexpr int N_AUX = 2;
    struct Stage { const char* name; std::function<int()> launch; int aux = 0; int join = 0; };
    std::vector<Stage> stages;
    virtual int use() = 0;
    virtual rt::Stream& stream() = 0;
    virtual rt::Stream& stream_aux(int k = 1) = 0;
    virtual int fork_aux(int k = 1) = 0;         // side stream k waits for what the main stream has issued
    virtual int join_aux(int k = 1) = 0;         // main stream waits for what side stream k has issued
    virtual int sync_aux() = 0;                  // host waits for every side stream that exists
    virtual int reset() = 0;                     // restore the pre-run status so the job can run again
    virtual int fetch_status(int8_t*) = 0;
    // submit form (bbs_core_*_submit): the statuses are copied to page-locked memory behind the last stage, and
    // wait() hands them to the caller's buffer `deliver_to`
    int8_t* deliver_to = nullptr;
    virtual int enqueue_status_fetch() = 0;
    virtual int deliver() = 0;
    // sign / proof_gen: the produced records follow the statuses to page-locked memory; deliver() unpacks them into the
    // caller's buffers
    virtual int enqueue_result_fetch() { return BBS_OK; }
    virtual void set_result_targets(uint8_t*, uint8_t*, uint64_t*) {}
    virtual int set_octet_form() { return BBS_E_ARG; }    // sign / proof_gen: results leave as octet strings (before run)
    virtual size_t device_bytes() const { return 0; }     // device memory this job holds (allocation size classes)
    // bbs_job_bv_report: set by a job with combined checks -- a keyed job that formed groups (job_form.hpp add_keyed_bv_stages)
    // or a single-key batch-verification job (add_batch_combination: one group of all n items); neither: zeros
    std::function<int(uint32_t*, uint32_t*, uint32_t*)> bv_report;
    // bbs_job_bv_verdicts: the raw verdict flags of the last run, read back on request (set where bv_report is): 16 per group
    std::function<int(std::vector<int8_t>&)> bv_verdicts;
    // bbs_job_key_statuses: set by a job with a job-local key set (job_form.hpp JobKeys): KeyBuild's code per key, read back on request
    std::function<int(std::vector<int8_t>&)> key_statuses;
    // bbs_job_key_cache_report: a job that came through a bbs_*_with_keys_* export says what the job-local key cache did for it
    bool has_job_keys = false, key_cache_bypassed = false;
    uint32_t key_cache_hits = 0, key_cache_misses = 0;
    virtual int fetch_signatures(uint8_t*) { return BBS_E_ARG; }
    virtual int fetch_proofs(uint8_t*, uint8_t*, uint64_t*) { return BBS_E_ARG; }
    // One pass over the stages.  ev != nullptr: one event before the first stage, then a (start, stop) pair around
    // every stage, each recorded on the stream that stage is launched on (1 + 2 * stages events per pass).
    int run_recorded(rt::EventList* ev) {
        if (reset()) return BBS_E_HIP;
        if (ev && ev->record(stream())) return BBS_E_HIP;
        unsigned forked = 0;
        // FAULT INJECTION for the fail-closed tests (tests/parity_cases.py::check_fail_closed_submit): the stages named in
        // BBS_FAULT_SKIP_STAGE (comma-separated) are not launched, so the items they would have decided stay undecided and
        // every way out of the library must refuse with BBS_E_STATE.  Read at every run; unset in any real deployment.
        const char* skip = getenv("BBS_FAULT_SKIP_STAGE");
        auto skipped = [skip](const char* name) {
            if (!skip || !*skip) return false;
            const size_t len = std::strlen(name);
            for (const char* p = skip; (p = std::strstr(p, name)) != nullptr; p += len)
                if ((p == skip || p[-1] == ',') && (p[len] == 0 || p[len] == ',')) return true;
            return false;
        };
        for (auto& s : stages) {
            if (s.aux < 0 || s.aux > N_AUX) return BBS_E_STATE;
            if (skipped(s.name)) continue;
            if (s.aux && !((forked >> s.aux) & 1u)) { if (fork_aux(s.aux)) return BBS_E_HIP; forked |= 1u << s.aux; }
            for (int k = 1; k <= N_AUX; k++)
                if (((s.join >> (k - 1)) & 1) && ((forked >> k) & 1u)) { if (join_aux(k)) return BBS_E_HIP; }
            rt::Stream& st = s.aux ? stream_aux(s.aux) : stream();
            if (ev && ev->record(st)) return BBS_E_HIP;
            if (s.launch()) return BBS_E_HIP;
            if (ev && ev->record(st)) return BBS_E_HIP;
        }
        return BBS_OK;
    }
    bool timed = false;                          // set from bbs_ctx::stage_timing when the job is created
    std::unique_ptr<rt::EventList> tev;          // events of the LAST run (timed jobs)
    bool results_wanted = false;                 // submit form of sign / proof_gen: the records follow the statuses
    int run() {
        failed.store(false, std::memory_order_release);
        if (use()) { mark_failed(false); return BBS_E_HIP; }
        if (timed) tev.reset(new rt::EventList(1 + 2 * stages.size()));
        int rc = run_recorded(timed ? tev.get() : nullptr);
        // a submit-form job that is run AGAIN (bbs_job_run): what bbs_job_wait delivers must be this run's statuses and
        // records, not the first run's -- the copies to page-locked memory are enqueued behind every run
        if (!rc && deliver_to) {
            rc = enqueue_status_fetch();
            if (!rc && results_wanted) rc = enqueue_result_fetch();
        }
        if (!rc && !hold_arm) rc = arm_completion();
        else if (rc) mark_failed(false);
        return rc;
    }
    // stage durations of the last run of a timed job; call after wait()
    int stage_times(float* total_ms, float* kernel_ms, int cap, int* n_stages) {
        const int ns = (int)stages.size();
        if (n_stages) *n_stages = ns;
        if (!timed || !tev || tev->used != 1 + 2 * (size_t)ns) return BBS_E_STATE;
        if (use() || rt::sync(stream()) || sync_aux()) return BBS_E_HIP;
        if (total_ms) *total_ms = tev->ms(0, 2 * (size_t)ns);
        for (int k = 0; kernel_ms && k < ns && k < cap; k++) kernel_ms[k] = tev->ms(1 + 2 * (size_t)k, 2 + 2 * (size_t)k);
        return BBS_OK;
    }
    int wait() {
        if (use() || rt::sync(stream())) return BBS_E_HIP;
        if (failed.load(std::memory_order_acquire)) return BBS_E_HIP;     // the last run was not enqueued completely: nothing to deliver
        return deliver_to ? deliver() : BBS_OK;
    }
};

template <class C>
struct JobBase : bbs_job {
    Ctx<C>* ctx;
    DevBuf d_status, d_status0;      // per-item statuses; d_status0 = what the ingest stage decided (restored before every run)
    HostBuf h_status;                // page-locked landing area of the submit form
    // the batch as the caller handed it over: page-locked image (source of the ONE asynchronous H2D copy) and the same
    // image on the device, which the ingest stage reads and where headers / presentation headers stay.  Members of
    // this base so that they outlive the destructor's stream synchronisation.
    HostBuf h_raw;
    DevBuf d_raw;
    std::vector<std::pair<void*, size_t>> zero_on_reset;   // device arrays cleared before every run (fail closed)
    std::vector<std::unique_ptr<DevBuf>> bufs;
    std::shared_ptr<const void> key_set;     // keyed jobs: the context's key set at upload (released after the streams synchronised)
    std::shared_ptr<const void> len_set;     // mixed-length jobs: the context's per-length domain prefixes at upload (likewise)
    std::shared_ptr<const void> key_len_set; // keyed jobs of mixed counts: the prefixes per (key, length) at upload (likewise)
    std::shared_ptr<const void> key_blob;    // jobs with a job-local key set: what their keys were hashed with (likewise)
    std::shared_ptr<void> key_cache_pin;     // cached jobs: the generation they read and their pins on its slots (likewise)
    std::shared_ptr<const void> sign_key_set;// keyed sign jobs: the context's signing set at upload (likewise; the last holder clears it)
    // every job owns its streams: independent jobs (batches) of one context overlap on the GPU
    rt::Stream main{}, aux[bbs_job::N_AUX]{};
    rt::Event ev_fork[bbs_job::N_AUX]{}, ev_join[bbs_job::N_AUX]{};
    bool main_ready = false, aux_ready[bbs_job::N_AUX] = {false, false};
    bool aux_shared[bbs_job::N_AUX] = {false, false};      // the queue budget left no stream for this side stream: its stages run on the main stream
    bool latency_form = false;       // decided when the job is created (Ctx::latency_form_now)
    explicit JobBase(Ctx<C>* c) : ctx(c) {
        main_ready = (ctx->use() == 0) && (rt::stream_create(&main) == 0); timed = c->stage_timing;
        ctx->live_jobs.fetch_add(1);
        device_live_jobs(ctx->device).fetch_add(1);
        latency_form = ctx->latency_form_now();
    }
    ~JobBase() override {
        ctx->live_jobs.fetch_sub(1);
        device_live_jobs(ctx->device).fetch_sub(1);
        (void)ctx->use();            // streams and buffers go back to this device's pools
        for (int k = 0; k < bbs_job::N_AUX; k++)
            if (aux_ready[k]) { rt::sync(aux[k]); rt::event_destroy(ev_fork[k]); rt::event_destroy(ev_join[k]); rt::stream_destroy(aux[k]); }
        if (main_ready) { rt::sync(main); rt::stream_destroy(main); }
    }
    int use() override { return ctx->use(); }
    size_t device_bytes() const override {
        size_t t = 0;
        auto add = [&](const DevBuf& b) { if (b.p) t += rt::size_class(b.bytes); };
        add(d_status); add(d_status0); add(d_raw);
        for (const auto& b : bufs) add(*b);
        return t;
    }
    rt::Stream& stream() override { return main_ready ? main : ctx->stream; }
    int ensure_aux(int k) {                      // k = 1 .. N_AUX
        if (k < 1 || k > bbs_job::N_AUX) return -1;
        if (aux_ready[k - 1] || aux_shared[k - 1]) return 0;
        const int rc = rt::stream_create(&aux[k - 1]);
        if (rc == -2) { aux_shared[k - 1] = true; return 0; }     // over the queue budget: share the main stream (in order, no fork / join)
        if (rc) return -1;
        if (rt::event_create(&ev_fork[k - 1])) { rt::stream_destroy(aux[k - 1]); return -1; }
        if (rt::event_create(&ev_join[k - 1])) { rt::event_destroy(ev_fork[k - 1]); rt::stream_destroy(aux[k - 1]); return -1; }
        aux_ready[k - 1] = true;
        return 0;
    }
    rt::Stream& stream_aux(int k = 1) override { ensure_aux(k); return (k >= 1 && k <= bbs_job::N_AUX && aux_ready[k - 1]) ? aux[k - 1] : stream(); }
    int fork_aux(int k = 1) override {
        if (ensure_aux(k)) return -1;
        if (!aux_ready[k - 1]) return 0;
        return (rt::event_record(ev_fork[k - 1], stream()) || rt::stream_wait(aux[k - 1], ev_fork[k - 1])) ? -1 : 0;
    }
    int join_aux(int k = 1) override {
        if (ensure_aux(k)) return -1;
        if (!aux_ready[k - 1]) return 0;
        return (rt::event_record(ev_join[k - 1], aux[k - 1]) || rt::stream_wait(stream(), ev_join[k - 1])) ? -1 : 0;
    }
    int sync_aux() override {
        int rc = 0;
        for (int k = 0; k < bbs_job::N_AUX; k++) if (aux_ready[k] && rt::sync(aux[k])) rc = -1;
        return rc;
    }
    // device-to-device, asynchronous: back-to-back runs of one job never wait for the host
    int reset() override {
        if (rt::d2d_async(d_status.p, d_status0.p, n, stream())) return BBS_E_HIP;
        for (auto& z : zero_on_reset) if (rt::dmemset(z.first, 0, z.second, stream())) return BBS_E_HIP;
        return BBS_OK;
    }
    int fetch_status(int8_t* out) override {
        if (use() || rt::sync(stream())) return BBS_E_HIP;
        if (rt::d2h(out, d_status.p, n, stream())) return BBS_E_HIP;
        return statuses_final(out, n) ? BBS_OK : BBS_E_STATE;
    }
    // the stream has been synchronised: BBS_E_STATE unless every item of the last run has been decided.  The record
    // buffers of sign / proof_gen are written by the last stage of a run; before that they hold whatever the pooled
    // allocation held, which must never reach a caller.
    int require_decided() {
        std::vector<int8_t> st(n);
        if (n && rt::d2h(st.data(), d_status.p, n, stream())) return BBS_E_HIP;
        return statuses_final(st.data(), n) ? BBS_OK : BBS_E_STATE;
    }
    int enqueue_status_fetch() override {
        if (!h_status.p && h_status.alloc(n ? n : 1)) return BBS_E_NOMEM;
        return rt::d2h_async(h_status.p, d_status.p, n, stream()) ? BBS_E_HIP : BBS_OK;
    }
    int deliver() override {                       // the stream has been synchronised
        if (!h_status.p) return BBS_E_STATE;
        if (!statuses_final(h_status.template as<int8_t>(), n)) return BBS_E_STATE;
        if (n) std::memcpy(deliver_to, h_status.p, n);
        return BBS_OK;
    }
    // upload a host vector, return device pointer (owned by the job)
    template <class T>
    T* up(const std::vector<T>& v, int& rc) {
        bufs.emplace_back(new DevBuf());
        DevBuf& b = *bufs.back();
        if (b.alloc(v.size() * sizeof(T))) { rc = BBS_E_NOMEM; return nullptr; }
        if (rt::h2d(b.p, v.data(), v.size() * sizeof(T), stream())) { rc = BBS_E_HIP; return nullptr; }
        return b.as<T>();
    }
    template <class T>
    T* scratch(size_t count, int& rc) {
        bufs.emplace_back(new DevBuf());
        DevBuf& b = *bufs.back();
        if (b.alloc(count * sizeof(T))) { rc = BBS_E_NOMEM; return nullptr; }
        return b.as<T>();
    }
    // the initial statuses come from the device's ingest stage (no host validation pass, no synchronous copy)
    int finish_setup_device() {
        if (d_status.alloc(n ? n : 1) || d_status0.alloc(n ? n : 1)) return BBS_E_NOMEM;
        if (rt::dmemset(d_status.p, (uint8_t)ST_PENDING, n, stream())) return BBS_E_HIP;
        return ctx->sync_consts();
    }
    template <class T>
    int down(std::vector<T>& v, const T* dptr) {
        return rt::d2h(v.data(), dptr, v.size() * sizeof(T), stream()) ? BBS_E_HIP : BBS_OK;
    }
};


// =============================================================================================
// staging image: the batch as the caller handed it over, one page-locked buffer, one asynchronous copy
// =============================================================================================
// Ragged input arrays of one batch inside the staging image: offsets rebased to 0, sections 16-byte aligned.
// offsets of a ragged section without entries (a batch without messages): one zero that may be read at index 0
inline const uint64_t* zero_off1() { static const uint64_t z[1] = {0}; return z; }
struct RaggedIn {
    const uint64_t* off;      // n + 1 caller offsets, or nullptr (every item empty)
    const uint8_t* data;
    size_t elem;              // bytes per element
    uint64_t total = 0;       // elements
    size_t at_off = 0, at_data = 0;
    bool offsets_only = false; // the elements themselves are produced on the device (no data behind the offsets)
    // false: offsets decrease, or data missing
    bool measure(size_t n) {
        total = 0;
        if (!off) return true;
        for (size_t i = 0; i < n; i++) if (off[i + 1] < off[i]) return false;
        total = off[n] - off[0];
        if (total > ((uint64_t)1 << 36)) return false;       // no batch holds 2^36 elements: garbage offsets, and total * elem must not wrap
        return total == 0 || data != nullptr || offsets_only;
    }
    void place(size_t& cur, size_t n) {
        at_off = cur; cur += ((n + 1) * 8 + 15) & ~(size_t)15;
        at_data = cur; if (!offsets_only) cur += ((size_t)total * elem + 4 + 15) & ~(size_t)15;
    }
    void fill(uint8_t* img, size_t n) const {
        uint64_t* o = reinterpret_cast<uint64_t*>(img + at_off);
        if (!off) { std::memset(o, 0, (n + 1) * 8); return; }
        const uint64_t b = off[0];
        for (size_t i = 0; i <= n; i++) o[i] = off[i] - b;
        if (total && !offsets_only) std::memcpy(img + at_data, data + b * elem, (size_t)total * elem);
    }
};

// Fixed-size records at the start of the image + the ragged sections behind them; allocates the job's page-locked and
// device buffers, fills the host image and enqueues the ONE host-to-device copy on the job's stream.
template <class J>
inline int stage_image(J* job, size_t n, const uint8_t* records, size_t rec_bytes, std::initializer_list<RaggedIn*> sections,
                       RaggedIn* extra = nullptr, size_t extra_count = 0,        // extra: a section ragged over extra_count entries
                       const std::vector<uint32_t>* words = nullptr, size_t* words_at = nullptr) {   // words: appended, at *words_at
    size_t cur = (n * rec_bytes + 15) & ~(size_t)15;
    for (RaggedIn* s : sections) s->place(cur, n);
    if (extra) extra->place(cur, extra_count);
    if (words) { *words_at = cur; cur += (words->size() * 4 + 15) & ~(size_t)15; }
    if (job->h_raw.alloc(cur) || job->d_raw.alloc(cur)) return BBS_E_NOMEM;
    uint8_t* img = job->h_raw.template as<uint8_t>();
    if (n && rec_bytes) std::memcpy(img, records, n * rec_bytes);
    for (RaggedIn* s : sections) s->fill(img, n);
    if (extra) extra->fill(img, extra_count);
    if (words && !words->empty()) std::memcpy(img + *words_at, words->data(), words->size() * 4);
    return rt::h2d_async(job->d_raw.p, img, cur, job->stream()) ? BBS_E_HIP : BBS_OK;
}

// The raw-message section `mb` of an upload (msg_byte_off != nullptr: the messages arrive as raw bytes) and nm, the messages of
// the whole batch (0: scalars).  `items` is the measured per-item section of message counts: message t of the batch is entry
// items.off[0] + t of msg_byte_off (item offsets need not start at zero; nm == 0: msg_byte_off is never indexed).  The section
// is ragged over MESSAGES, not items: stage_image places and fills it with nm as its count.  false: BBS_E_ARG.
inline bool raw_message_section(const RaggedIn& items, const uint64_t* msg_byte_off, const uint8_t* msg_bytes, RaggedIn& mb, size_t& nm) {
    const bool raw = msg_byte_off != nullptr;
    nm = raw ? (size_t)items.total : 0;
    mb = RaggedIn{raw ? (nm ? msg_byte_off + items.off[0] : zero_off1()) : nullptr, msg_bytes, 1};
    return !raw || (mb.measure(nm) && mb.total <= 0xF0000000ull);
}
// the GLV split of a variable-base scalar is sound for points of the subgroup: always (BN254), on the caller's word, or in the
// wire forms, where the decoder has checked every point
template <class C>
inline int glv_flag(const Ctx<C>* ctx, bool wire) {
    return (C::K::HAS_GLV && (C::K::GLV_ALWAYS || ctx->points_in_subgroup || wire)) ? 1 : 0;
}

// msg_to_scalars on the device (codec_dev.hpp MsgHash): the nm raw messages of a batch, placed in the staging image as
// section `mb`, become nm canonical scalars [message][8 words] -- the array the ingest stages read messages from.
// dst_too_long = 1 (and no launch): api_id || "MAP_MSG_TO_SCALAR_AS_HASH_" exceeds 255 bytes, the reference panics.
template <class C, class J>
inline uint32_t* hash_raw_messages(J* job, Ctx<C>* ctx, const RaggedIn& mb, size_t nm, MsgHashArgs& ma, int& dst_too_long, int& rc) {
    static const char SUFFIX[] = "MAP_MSG_TO_SCALAR_AS_HASH_";
    const size_t dl = ctx->api_id.size() + sizeof(SUFFIX) - 1;
    uint32_t* out = job->template scratch<uint32_t>(std::max<size_t>(nm, 1) * 8, rc);
    if (rc) return nullptr;
    dst_too_long = dl > 255 ? 1 : 0;
    if (dst_too_long || !nm) return out;
    const uint8_t* dimg = job->d_raw.template as<uint8_t>();
    std::memset(&ma, 0, sizeof(ma));
    ma.nm = nm; ma.off = reinterpret_cast<const uint64_t*>(dimg + mb.at_off); ma.bytes = dimg + mb.at_data; ma.out = out;
    std::memcpy(ma.dst, ctx->api_id.data(), ctx->api_id.size());
    std::memcpy(ma.dst + ctx->api_id.size(), SUFFIX, sizeof(SUFFIX) - 1);
    ma.dst_len = (uint32_t)dl;
    if (rt::launch<MsgHash<C>>(job->stream(), ma, nm)) rc = BBS_E_HIP;
    return out;
}

// =============================================================================================
// batch verification plumbing shared by proof_verify and verify (pippenger.hpp)
// =============================================================================================
template <class C>
struct BvState {
    RlcPrepArgs<C> prep{};
    PipArgs<C> pip{};            // host twin: the lane-per-bucket stages
    PipCoopArgs<C> coop{};       // device: the workgroup-cooperative kernel
    PipTileSumArgs<C> tsum{};
    const int8_t* batch_ok = nullptr;      // [n_checks] verdicts of the combined checks
    int n_checks = 0;
    PairArgs<C> pa_sum{};
};

#if !defined(BBS_HOST_TWIN)
namespace rt {
template <class C> struct PipKernelEntry { static const int token; };
template <class C> const int PipKernelEntry<C>::token = register_kernel(reinterpret_cast<const void*>(&k_pip_window<C>));
template <class C>
inline int launch_pip_windows(Stream& s, const PipCoopArgs<C>& a) {
    const size_t units = (size_t)a.M * a.NW * a.n_tiles;
    (void)&PipKernelEntry<C>::token;
    if (!units || !a.n) return 0;
    hipLaunchKernelGGL((k_pip_window<C>), dim3((unsigned)units), dim3(PIP_WG), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// the segmented form (keyed batch verification): used, and so instantiated, by the keyed translation units only
template <class C> struct PipSegKernelEntry { static const int token; };
template <class C> const int PipSegKernelEntry<C>::token = register_kernel(reinterpret_cast<const void*>(&k_pip_window_seg<C>));
template <class C>
inline int launch_pip_window_segs(Stream& s, const PipSegArgs<C>& a) {
    const size_t units = (size_t)a.M * a.NW * a.n_segs;
    (void)&PipSegKernelEntry<C>::token;
    if (!units) return 0;
    if (units > 0x7FFFFFFFull) return -1;
    hipLaunchKernelGGL((k_pip_window_seg<C>), dim3((unsigned)units), dim3(PIP_WG), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
}  // namespace rt

// The six-lane pairing kernels take the form of the line tables as a template parameter: launch_line_form is the one place
// that turns the run-time `unit` into it.  The launchers of the single-key kernels (stages_pair.hpp) follow, with the geometry
// of pairing_dist.hpp; the keyed one is job_form.hpp launch_pair_fused_keyed.
template <template <class, bool> class K, class C, class A>
inline int launch_line_form(rt::Stream& st, bool unit, const A& a, size_t nthreads) {
    return unit ? rt::launch<K<C, true>>(st, a, nthreads) : rt::launch<K<C, false>>(st, a, nthreads);
}
template <class C>
inline int launch_pair_fused(rt::Stream& st, bool unit, const PairArgs<C>& a) {
    return launch_line_form<PairDist, C>(st, unit, a, pair6_threads(a.n));
}
template <class C>
inline int launch_pair_miller_split(rt::Stream& st, bool unit, const PairArgs<C>& a) {
    return launch_line_form<PairMillerHalf, C>(st, unit, a, pair6_split_threads(a.n));
}
template <class C>
inline int launch_pair_final(rt::Stream& st, const PairArgs<C>& a) {
    return rt::launch<PairFinalDist<C>>(st, a, pair6_threads(a.n));
}
#endif

// one pairing product check as stages on the job's main (aux = 0) or second stream.  Split: the two Miller loops of an
// item on separate wavefronts and the final exponentiation as its own stage; fused: one kernel.  (The host twin runs its
// one-lane pair of stages whatever is asked: it uses neither nm_dist nor split, hence [[maybe_unused]].)
enum class PairSplit {
    ByJobForm,   // split in the job's latency form, fused in the throughput form
    Always,      // the sixteen combined checks of batch verification, which are the narrow tail of their job
    Never,       // proof_verify (see op_pv.hpp)
};
template <class C, class J>
void add_pairing_stages(J* j, PairArgs<C>* pargs, int aux, const char* nm_miller, const char* nm_final, [[maybe_unused]] const char* nm_dist,
                        [[maybe_unused]] PairSplit split = PairSplit::ByJobForm,
                        int join_first = 0) {       // join_first: the (main-stream) first stage waits for the second stream
    const size_t first = j->stages.size();
    struct JoinFirst { J* j; size_t first; int join; ~JoinFirst() { if (join && j->stages.size() > first) j->stages[first].join = 1; } } jf{j, first, join_first};
#ifdef BBS_HOST_TWIN
    j->stages.push_back({nm_miller, [j, pargs, aux]() { return rt::launch<PairMiller<C>>(aux ? j->stream_aux() : j->stream(), *pargs, pargs->n * 2); }, aux, 0});
    j->stages.push_back({nm_final, [j, pargs, aux]() { return rt::launch<PairFinal<C>>(aux ? j->stream_aux() : j->stream(), *pargs, pargs->n); }, aux, 0});
#else
    if (split == PairSplit::Always || (split == PairSplit::ByJobForm && j->latency_form)) {
        // the two Miller loops of every item on separate wavefronts, then product + final exponentiation (stages.hpp)
        j->stages.push_back({nm_miller, [j, pargs, aux]() { return launch_pair_miller_split<C>(aux ? j->stream_aux() : j->stream(), j->ctx->dev_lines_unit, *pargs); }, aux, 0});
        j->stages.push_back({nm_final, [j, pargs, aux]() { return launch_pair_final<C>(aux ? j->stream_aux() : j->stream(), *pargs); }, aux, 0});
        return;
    }
    j->stages.push_back({nm_dist, [j, pargs, aux]() { return launch_pair_fused<C>(aux ? j->stream_aux() : j->stream(), j->ctx->dev_lines_unit, *pargs); }, aux, 0});
#endif
}

// Batch verification (pippenger.hpp), in two parts so that a job can place them on different streams:
//   add_batch_combination : RlcPrep (coefficients, the two point sets item-major), the bucket-method sums of both sets per
//                           8-bit window, and the 16 pairing products  e(sum_w pts0, pk) e(+-sum_w pts1, BP2)  side by side
//                           -- on the job's second stream (aux = 1: proof_verify, whose points are inputs) or on the main one;
//   add_batch_decision    : (main stream; joins the second) the per-item kernel `fallback` (gate: status == ST_PAIRING) with the
//                           16 verdicts: all 1 -> its lanes write Ok(true) and return, otherwise they compute the item's own product.
template <class C, class J>
int add_batch_combination(J* j, BvState<C>* bv, Ctx<C>* ctx, size_t n, const CtxConsts<C>* cc, const uint32_t* pa, const uint32_t* pb,
                          int canonical, const int8_t* gate_arr, int gate, int negate_b, int aux, bool with_prep = true) {
    constexpr int N = C::FpP::N;
    constexpr int NW = 16, M = 2;
    const size_t n_pad = (n + 3) & ~(size_t)3, nn = std::max<size_t>(n, 1);
    int rc = BBS_OK;
    RlcPrepArgs<C>& pr = bv->prep;
    uint8_t* dig = j->template scratch<uint8_t>((size_t)NW * n_pad + 4, rc);
    uint32_t* ppts = j->template scratch<uint32_t>((size_t)M * nn * 2 * N, rc);
    uint32_t* out = j->template scratch<uint32_t>((size_t)M * 2 * N * NW, rc);          // [M][2N][NW]: NW affine sums per set
    // [0 .. NW) gates of the NW combined checks (all 1), [NW .. 2 NW) their results
    std::vector<int8_t> fl(2 * NW, 0);
    for (int k = 0; k < NW; k++) fl[k] = 1;
    int8_t* flags = j->up(fl, rc);
    uint32_t* fm_sum = j->template scratch<uint32_t>((size_t)2 * 12 * N * NW, rc);
    if (rc) return rc;
    if (rt::dmemset(dig, 0, (size_t)NW * n_pad, j->stream())) return BBS_E_HIP;
    j->zero_on_reset.push_back({flags + NW, (size_t)NW});          // a combined check that never ran reads as failed
    pr.n = n; pr.n_pad = n_pad; pr.pa = pa; pr.pb = pb; pr.canonical = canonical; pr.gate_arr = gate_arr; pr.gate = gate;
    pr.dig = dig; pr.ppts = ppts;
    ctx->next_rlc_seed(pr.seed);
    bv->batch_ok = flags + NW; bv->n_checks = NW;
    PairArgs<C>& ps = bv->pa_sum;
    ps.n = NW; ps.cc = cc; ps.pa = out; ps.pb = out + (size_t)2 * N * NW; ps.negate_b = negate_b; ps.canonical = 0;
    ps.gate_arr = flags; ps.gate = 1; ps.out = flags + NW; ps.fmiller = fm_sum;
    auto strm = [j, aux]() -> rt::Stream& { return aux ? j->stream_aux() : j->stream(); };
    // with_prep = false: the caller's own stage writes the digits and the item-major points (proof_verify's PvChallengeBv)
    if (with_prep) j->stages.push_back({"rlc_prep", [j, bv, strm]() { return rt::launch<RlcPrep<C>>(strm(), bv->prep, j->n); }, aux, 0});
#ifdef BBS_HOST_TWIN
    PipArgs<C>& pp = bv->pip;
    pp.n = n; pp.n_pad = n_pad; pp.M = M; pp.NW = NW; pp.ppts = ppts; pp.dig = dig; pp.out = out;
    pp.list = j->template scratch<uint32_t>((size_t)M * NW * nn, rc);
    pp.buckets = j->template scratch<uint32_t>((size_t)3 * N * M * NW * PIP_NB, rc);
    pp.segs = j->template scratch<uint32_t>((size_t)3 * N * M * NW * (PIP_NB / PIP_SEG), rc);
    pp.wins = j->template scratch<uint32_t>((size_t)3 * N * M * NW, rc);
    if (rc) return rc;
    j->stages.push_back({"pip_buckets", [bv, strm]() { return rt::launch<PipBuckets<C>>(strm(), bv->pip, (size_t)bv->pip.M * bv->pip.NW * PIP_NB); }, aux, 0});
    j->stages.push_back({"pip_segments", [bv, strm]() { return rt::launch<PipSegments<C>>(strm(), bv->pip, (size_t)bv->pip.M * bv->pip.NW * (PIP_NB / PIP_SEG)); }, aux, 0});
    j->stages.push_back({"pip_window_sums", [bv, strm]() { return rt::launch<PipWindowSums<C>>(strm(), bv->pip, (size_t)bv->pip.M * bv->pip.NW); }, aux, 0});
#else
    PipCoopArgs<C>& co = bv->coop;
    co.n = n; co.n_pad = n_pad; co.M = M; co.NW = NW; co.n_tiles = (int)((nn + PIP_TILE - 1) / PIP_TILE); co.ppts = ppts; co.dig = dig;
    co.tile_sums = j->template scratch<uint32_t>((size_t)3 * N * M * NW * co.n_tiles, rc);
    if (rc) return rc;
    PipTileSumArgs<C>& ts = bv->tsum;
    ts.M = M; ts.NW = NW; ts.n_tiles = n ? co.n_tiles : 0; ts.shift = 0; ts.tile_sums = co.tile_sums; ts.out = out; ts.wins = nullptr;
    co.out_aff = (n && co.n_tiles == 1) ? out : nullptr;      // one tile: the kernel's thread 0 normalises the window sum itself
    j->stages.push_back({"pip_windows", [bv, strm]() { return rt::launch_pip_windows<C>(strm(), bv->coop); }, aux, 0});
    if (!co.out_aff)
        j->stages.push_back({"pip_tile_sums", [bv, strm]() { return rt::launch<PipTileSums<C>>(strm(), bv->tsum, (size_t)bv->tsum.M * bv->tsum.NW); }, aux, 0});
#endif
    add_pairing_stages<C>(j, &bv->pa_sum, aux, "rlc_pair_miller", "rlc_pair_final_exp", "rlc_pairing_6lane", PairSplit::Always);
    // bbs_job_bv_verdicts / bbs_job_bv_report: the 16 results as the decision reads them (the second stream has been joined by
    // the time the job is waited for); the report counts the whole job as one group
    j->bv_verdicts = [j, flags](std::vector<int8_t>& v) {
        v.assign(NW, 0);
        if (j->use() || rt::sync(j->stream())) return (int)BBS_E_HIP;
        return rt::d2h(v.data(), flags + NW, v.size(), j->stream()) ? (int)BBS_E_HIP : (int)BBS_OK;
    };
    j->bv_report = [j](uint32_t* groups, uint32_t* passed, uint32_t* items) {
        std::vector<int8_t> v;
        if (const int rc = j->bv_verdicts(v)) return rc;
        bool all = true;
        for (const int8_t f : v) all &= f == 1;
        *groups = 1; *passed = all ? 1u : 0u; *items = (uint32_t)j->n;
        return (int)BBS_OK;
    };
    return BBS_OK;
}
template <class C, class J>
void add_batch_decision(J* j, BvState<C>* bv, PairArgs<C>* fallback, int joins_aux) {
    // no kernel of its own: the per-item kernel's lanes read the 16 verdicts first -- all passed: write Ok(true) and leave
    fallback->batch_ok = bv->batch_ok; fallback->n_checks = bv->n_checks;
    add_pairing_stages<C>(j, fallback, 0, "fallback_pair_miller", "fallback_pair_final_exp", "fallback_pairing_6lane", PairSplit::ByJobForm, joins_aux);
}
