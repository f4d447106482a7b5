/* mm_hostcopy_plan.h -- the arithmetic and the ordering protocol of the staged device-to-host copy (mm_hostcopy.hip): when a copy
 * is staged, how many copy threads it takes, which bytes are chunk i, which of them thread t copies, and the loop that hands the
 * ring's slots from the DMA driver to the copy threads and back.  The protocol is a template over a TRANSPORT, the two calls
 * that start a DMA and ask whether it has finished; the library's transport is HIP's (mm_hostcopy.hip), the one of
 * tests/cpp/hostcopy_ring.cpp is a memcpy, so the whole protocol runs under the thread and address sanitizers without a GPU.
 * No HIP include; internal linkage: nothing here joins the library's exported symbols. */
#ifndef MM_HOSTCOPY_PLAN_H
#define MM_HOSTCOPY_PLAN_H

#include <sched.h>

#include <atomic>
#include <cstddef>
#include <cstring>
#include <thread>
#include <vector>

constexpr size_t kHostcopyChunk = 8u << 20; /* 0.15 ms of DMA per chunk: the ring's latency; 4 chunks in flight */
constexpr int kHostcopyRing = 4;
constexpr size_t kHostcopyDirectBelow = 4u << 20; /* small results: the plain copy (its staging inside the runtime is as good) */

/* The copy threads of ONE staged copy: half the usable CPUs, at most 8, divided by `active`, the staged copies in flight in
 * this process at the moment this one enters (itself included), at least 1.  A copy keeps its count until it ends, so k copies
 * that enter together see active = 1 .. k and hold n + n/2 + n/3 + ... threads between them (n = 8: 8, 4, 2, 2, 1, 1, 1, 1 = 20,
 * and one more for every further copy), beside one DMA driver each: later copies take fewer threads, the sum is NOT bounded by
 * n (tests/cpp/hostcopy_ring.cpp holds the closed form). */
static inline int mm_hostcopy_threads(int cpus, int active)
{
    /* DRAM, not cores, is the limit from a handful of threads on; leave half the usable CPUs to the caller */
    int n = cpus / 2;
    n = n < 1 ? 1 : (n > 8 ? 8 : n);
    n = n / (active < 1 ? 1 : active);
    return n < 1 ? 1 : n;
}

/* one plain copy instead of the ring?  With one usable CPU a copy thread and the DMA driver would only take turns; a pinned
 * destination is what the DMA engine writes at full speed itself */
static inline bool mm_hostcopy_direct(size_t bytes, int cpus, bool dst_pinned)
{
    return bytes < kHostcopyDirectBelow || cpus < 2 || dst_pinned;
}

static inline size_t mm_hostcopy_chunks(size_t bytes, size_t chunk) { return (bytes + chunk - 1) / chunk; }

struct mm_hostcopy_span {
    size_t off, len;
};

/* chunk i of `bytes`: source and destination bytes [off, off + len) */
static inline mm_hostcopy_span mm_hostcopy_chunk(size_t bytes, size_t chunk, size_t i)
{
    const size_t off = i * chunk, len = (off + chunk <= bytes) ? chunk : bytes - off;
    return {off, len};
}

struct mm_hostcopy_slice {
    size_t a, b; /* thread t copies bytes [a, b) of the chunk, and nothing where a >= len */
};

/* slices on 4 KB boundaries: every destination page is faulted in and written by one thread */
static inline mm_hostcopy_slice mm_hostcopy_slice_of(size_t len, int T, int t)
{
    const size_t per = ((len + (size_t)T - 1) / (size_t)T + 4095) & ~(size_t)4095;
    const size_t a = (size_t)t * per, b = a + per < len ? a + per : len;
    return {a, b};
}

/* waiting: `pause` for the first few hundred polls (a chunk is 0.15 ms of DMA), then give the CPU away between polls */
struct mm_hostcopy_backoff {
    unsigned int spins = 0;
    void wait()
    {
        if (++spins < 256) {
#if defined(__x86_64__)
            __builtin_ia32_pause();
#endif
        } else {
            sched_yield();
        }
    }
    void reset() { spins = 0; }
};

/* what a transport's query() answers beside 0 (the slot is filled) and its own error codes, which are positive */
constexpr int kHostcopyNotReady = -1;

struct mm_hostcopy_result {
    bool started; /* false: the copy threads could not be started; nothing was issued, nothing written: make the plain copy */
    int error;    /* 0, or what the transport's issue() / query() answered */
};

struct mm_hostcopy_std_thread {
    template <class F>
    std::thread operator()(F &f, int t) const
    {
        return std::thread(f, t);
    }
};

/* `bytes` of the transport's source into `dst` through its ring of kHostcopyRing slots of `chunk` bytes, with T copy threads
 * beside the calling one, which drives the DMA ring.  The transport:
 *     const void *slot(int s)                     the address of slot s
 *     int issue(int s, size_t off, size_t len)    start filling slot s from source bytes [off, off + len); 0 or an error
 *     int query(int s)                            the last issue on slot s: 0 done, kHostcopyNotReady, or an error
 * issue and query are called by this thread only, chunk after chunk, each chunk's query only after its issue.
 * `spawn(worker, t)` returns the started std::thread of copy thread t, or throws. */
template <class Transport, class Spawn = mm_hostcopy_std_thread>
static mm_hostcopy_result mm_hostcopy_ring(Transport &tr, void *dst, size_t bytes, size_t chunk, int T, Spawn spawn = Spawn())
{
    const size_t n_chunks = mm_hostcopy_chunks(bytes, chunk);
    /* published: chunks whose DMA has finished (the workers may read them); consumed[i % kRing]: workers done with chunk i */
    std::atomic<size_t> published{0};
    std::atomic<unsigned int> consumed[kHostcopyRing];
    std::atomic<bool> failed{false};
    for (auto &c : consumed)
        c.store(0, std::memory_order_relaxed);
    auto worker = [&](int t) {
        mm_hostcopy_backoff bo;
        for (size_t i = 0; i < n_chunks; ++i) {
            bo.reset();
            while (published.load(std::memory_order_acquire) <= i) {
                if (failed.load(std::memory_order_relaxed))
                    return;
                bo.wait();
            }
            const mm_hostcopy_span c = mm_hostcopy_chunk(bytes, chunk, i);
            const mm_hostcopy_slice s = mm_hostcopy_slice_of(c.len, T, t);
            if (s.a < c.len)
                std::memcpy((char *)dst + c.off + s.a, (const char *)tr.slot((int)(i % kHostcopyRing)) + s.a, s.b - s.a);
            consumed[i % kHostcopyRing].fetch_add(1, std::memory_order_release);
        }
    };
    /* A host that cannot start threads (resource limits) gets the plain copy: nothing may throw across the C ABI */
    std::vector<std::thread> threads;
    try {
        threads.reserve((size_t)T);
        for (int t = 0; t < T; ++t)
            threads.push_back(spawn(worker, t));
    } catch (...) {
        failed.store(true, std::memory_order_relaxed);
        for (std::thread &th : threads)
            th.join();
        return {false, 0};
    }
    size_t issued = 0, pub = 0;
    int e = 0;
    mm_hostcopy_backoff bo;
    while (pub < n_chunks) {
        bool progressed = false;
        if (issued < n_chunks) {
            /* slot free: never used, or every worker is done with the chunk that used it */
            const bool slot_free = issued < (size_t)kHostcopyRing ||
                                   consumed[issued % kHostcopyRing].load(std::memory_order_acquire) >= (unsigned int)T;
            if (slot_free) {
                if (issued >= (size_t)kHostcopyRing)
                    consumed[issued % kHostcopyRing].store(0, std::memory_order_relaxed);
                const mm_hostcopy_span c = mm_hostcopy_chunk(bytes, chunk, issued);
                if ((e = tr.issue((int)(issued % kHostcopyRing), c.off, c.len)) != 0)
                    break;
                ++issued;
                progressed = true;
            }
        }
        if (pub < issued) {
            const int q = tr.query((int)(pub % kHostcopyRing));
            if (q == 0) {
                published.store(++pub, std::memory_order_release);
                progressed = true;
            } else if (q != kHostcopyNotReady) {
                e = q;
                break;
            }
        }
        if (progressed)
            bo.reset();
        else
            bo.wait();
    }
    if (e != 0)
        failed.store(true, std::memory_order_relaxed);
    for (std::thread &th : threads)
        th.join();
    return {true, e};
}

#endif /* MM_HOSTCOPY_PLAN_H */
