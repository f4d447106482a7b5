/*
 * mm_hostcopy.hip -- a device buffer into the caller's HOST array at the speed of the link, whatever the array is.
 *
 * The reference's `run` returns host arrays (ChainRunner::run -> Array3, core.rs:176-186; HMC::run's tensor is read back
 * by the caller, hmc.rs:137-158), and a caller's `Vec` / numpy array is PAGEABLE memory: one hipMemcpyAsync into it
 * moved config 3's 315 MB sample at 9.9 GB/s (31.8 ms next to a 0.18 ms kernel; profiles/r4z_pcie_inclusive.json), into
 * pinned memory at 52.7 GB/s (5.97 ms).  Here the library stages: the DMA engine fills a ring of library-owned PINNED
 * bounce buffers chunk by chunk while a few host threads copy the finished chunks into the destination (each thread its
 * own slice of every chunk, so the destination's page faults and the DRAM traffic are spread over cores).  A destination
 * that IS pinned (hipHostMalloc / hipHostRegister / torch's pin_memory) gets the one direct copy as before.
 *
 * One stager per device (its own buffers and lock: shards of a device group copy side by side over their own links).  A
 * copy that enters while others are in flight takes fewer copy threads -- half the usable CPUs, at most 8, divided by the
 * copies in flight when it enters -- and keeps them until it ends: eight shards entering together hold 8 + 4 + 2 + 2 + 1 + 1 +
 * 1 + 1 = 20 copy threads and 8 drivers, not 8 x (8 + 1), but the sum is not capped (mm_hostcopy_threads); waiting threads
 * yield the CPU after a short spin.  The 32 MB pinned ring of a device that has staged once stays with the process (freeing
 * pinned memory from a static destructor races the runtime's own teardown); hosts with a single usable CPU get the plain copy.
 *
 * The thresholds, the chunk and slice arithmetic and the ring's ordering protocol are mm_hostcopy_plan.h, host-only and run
 * under the thread sanitizer by tests/cpp/hostcopy_ring.cpp; here: the stager, the pinned-destination test and HIP's transport.
 */
#include "mm_hostcopy.h"

#include <sched.h>
#include <unistd.h>

#include <atomic>
#include <mutex>

#include "mm_hostcopy_plan.h"

namespace {

constexpr size_t kChunk = kHostcopyChunk;
constexpr int kRing = kHostcopyRing;

struct Stager {
    std::mutex mu;
    void *pin[kRing] = {};
    hipEvent_t ev[kRing] = {};
    bool ready = false;
};

Stager &stager(int device)
{
    static Stager s[64];
    return s[device & 63];
}

int usable_cpus()
{
    cpu_set_t set;
    int n = 0;
    if (sched_getaffinity(0, sizeof set, &set) == 0)
        n = CPU_COUNT(&set);
    if (n <= 0)
        n = (int)sysconf(_SC_NPROCESSORS_ONLN);
    return n < 1 ? 1 : n;
}

/* staged copies in flight in this process (the shards of a device group copy side by side): a copy that enters beside others
 * takes fewer copy threads (mm_hostcopy_threads) */
std::atomic<int> g_active{0};

bool is_pinned_host(const void *p)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError(); /* an ordinary malloc'ed pointer is "invalid value" to the runtime: not an error here */
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

struct ActiveGuard {
    int n;
    ActiveGuard() : n(g_active.fetch_add(1, std::memory_order_relaxed) + 1) {}
    ~ActiveGuard() { g_active.fetch_sub(1, std::memory_order_relaxed); }
};

/* the ring's transport: the DMA engine fills slot s on `stream`, an event per slot says when */
struct HipTransport {
    Stager &st;
    const void *d_src;
    hipStream_t stream;
    const void *slot(int s) const { return st.pin[s]; }
    int issue(int s, size_t off, size_t len)
    {
        hipError_t e;
        if ((e = hipMemcpyAsync(st.pin[s], (const char *)d_src + off, len, hipMemcpyDeviceToHost, stream)) != hipSuccess ||
            (e = hipEventRecord(st.ev[s], stream)) != hipSuccess)
            return (int)e;
        return 0;
    }
    int query(int s)
    {
        const hipError_t q = hipEventQuery(st.ev[s]);
        return q == hipSuccess ? 0 : q == hipErrorNotReady ? kHostcopyNotReady : (int)q;
    }
};

} // namespace

hipError_t mm_copy_to_host(void *dst, const void *d_src, size_t bytes, int device, hipStream_t stream)
{
    if (bytes == 0)
        return hipSuccess;
    hipError_t e;
    const int cpus = usable_cpus();
    /* the runtime is asked about the destination only where its answer decides */
    if (mm_hostcopy_direct(bytes, cpus, false) || mm_hostcopy_direct(bytes, cpus, is_pinned_host(dst))) {
        if ((e = hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, stream)) != hipSuccess)
            return e;
        return hipStreamSynchronize(stream);
    }
    ActiveGuard active;
    Stager &st = stager(device);
    std::lock_guard<std::mutex> lock(st.mu);
    if (!st.ready) {
        for (int i = 0; i < kRing; ++i) {
            if (!st.pin[i] && (e = hipHostMalloc(&st.pin[i], kChunk, hipHostMallocDefault)) != hipSuccess)
                return e;
            if (!st.ev[i] && (e = hipEventCreateWithFlags(&st.ev[i], hipEventDisableTiming)) != hipSuccess)
                return e;
        }
        st.ready = true;
    }
    /* T copy threads beside this one, which drives the DMA ring */
    HipTransport tr{st, d_src, stream};
    const mm_hostcopy_result r = mm_hostcopy_ring(tr, dst, bytes, kChunk, mm_hostcopy_threads(cpus, active.n));
    if (!r.started) {
        if ((e = hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, stream)) != hipSuccess)
            return e;
        return hipStreamSynchronize(stream);
    }
    e = (hipError_t)r.error;
    if (e != hipSuccess) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(stream); /* nothing of ours may still be in flight when the buffers are reused */
    }
    return e;
}
