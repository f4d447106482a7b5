/*
 * mm_group.hip -- device groups behind the C ABI: ONE call runs every chain on N GPUs of the process.
 *
 * The reference's contract is "run() executes all chains" (ChainRunner::run core.rs:176-186, HMC::run hmc.rs:137-158);
 * with one sampler handle per device the caller of the C ABI would have to write the sharding and the exchange of the
 * diagnostics itself.  A group owns one handle per device -- device i holds the contiguous block of global chains
 * [first_i, first_i + n_i), keyed into the random stream by their GLOBAL index, so the samples do not depend on the
 * number of devices.  `mmcmc_*_group_run` BLOCKS (whatever its arguments).  The asynchronous spelling is its own entry
 * point, `mmcmc_{mh,hmc}_group_run_async`: the launches are ENQUEUED on every shard's stream by the calling thread and
 * the call returns at once -- like the single-device call on a caller's stream, so back-to-back runs keep every device
 * busy without a host round trip per run (mmcmc_*_group_sync waits; everything that reads results is ordered behind the
 * queued work by the shard's stream).  Calls that block (group_run, NUTS with its adaptation hand-offs, the
 * diagnostics) run from one host thread per device, each blocking only its own thread.  A run that fails after some
 * shards have advanced and others have not marks the group broken (MMCMC_ERR_GROUP_BROKEN from then on).  Chains never talk to each other while sampling: no data-path collective.  The one exchange is
 * the split-R-hat / ESS reduction (stats.rs:416-546): every device reduces its own sample to the per-half-chain
 * statistics (mmcmc_stats_partials), RCCL all-gathers means / sums of squares over xGMI (ncclAllGather) and
 * all-reduces the lag sums (ncclAllReduce), and the host finish (mmcmc_stats_finish) runs on the gathered statistics
 * in the single-GPU order.  RCCL is loaded at run time (librccl.so.1: the copy PyTorch has already mapped, if any);
 * without it, or when a device appears twice in the list (several shards on one GPU: what a one-GPU test box can
 * exercise), the few KB of statistics are exchanged through the host instead.  mmcmc_group_bind_collectives binds the four
 * collective entry points from a library the caller names instead, before the first group exists; bound as accepting several
 * ranks on one device, a device listed twice keeps the collective branch (tests/c/fake_collectives.c: N > 1 ranks on one GPU).
 */
#include "../../include/mmcmc.h"
#include "mm_group_plan.h"
#include "mm_host.h"
#include "mm_hostcopy.h"
#include "mm_sampler_ops.h"

#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

namespace {

/* ---- the collectives (RCCL), bound at run time: once per process, by the first group that asks or -- before that -- by
 * mmcmc_group_bind_collectives from a library the caller names ---- */
typedef void *ncclComm_t;
struct Rccl {
    void *lib = nullptr;
    int (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
    int (*CommDestroy)(ncclComm_t) = nullptr;
    int (*AllGather)(const void *, void *, size_t, int, ncclComm_t, hipStream_t) = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
    bool ok() const { return CommInitAll && CommDestroy && AllGather && AllReduce; }
    /* the four entry points of an open library, by dlsym on THAT handle (not the process's first definition) */
    void take(void *handle)
    {
        lib = handle;
        CommInitAll = (int (*)(ncclComm_t *, int, const int *))dlsym(handle, "ncclCommInitAll");
        CommDestroy = (int (*)(ncclComm_t))dlsym(handle, "ncclCommDestroy");
        AllGather = (int (*)(const void *, void *, size_t, int, ncclComm_t, hipStream_t))dlsym(handle, "ncclAllGather");
        AllReduce = (int (*)(const void *, void *, size_t, int, int, ncclComm_t, hipStream_t))dlsym(handle, "ncclAllReduce");
    }
};
constexpr int kNcclFloat32 = 7, kNcclSum = 0;

struct Binding {
    std::mutex mu;
    bool bound = false;       /* decided for the life of the process (also when no library was found) */
    bool share_device = false; /* the bound library takes several ranks on one device */
    Rccl r;
};
Binding &binding()
{
    static Binding b;
    return b;
}

Rccl &rccl()
{
    Binding &b = binding();
    std::lock_guard<std::mutex> l(b.mu);
    if (!b.bound) {
        b.bound = true;
        void *lib = nullptr;
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (lib)
                break;
        }
        if (lib)
            b.r.take(lib);
    }
    return b.r; /* never changes once bound */
}

/* a device listed twice keeps the collectives only under a library bound as accepting that (RCCL does not) */
bool collectives_share_devices()
{
    Binding &b = binding();
    std::lock_guard<std::mutex> l(b.mu);
    return b.bound && b.share_device;
}

int bind_collectives(const char *library_path, int share_device)
{
    if (!library_path)
        return MMCMC_ERR_INVALID_ARG;
    Binding &b = binding();
    std::lock_guard<std::mutex> l(b.mu);
    if (b.bound)
        return MMCMC_ERR_INVALID_ARG;
    void *lib = dlopen(library_path, RTLD_NOW | RTLD_LOCAL);
    if (!lib)
        return MMCMC_ERR_INVALID_ARG;
    Rccl r;
    r.take(lib);
    if (!r.ok()) {
        dlclose(lib);
        return MMCMC_ERR_INVALID_ARG;
    }
    b.r = r;
    b.share_device = share_device != 0;
    b.bound = true;
    return MMCMC_OK;
}

/* withinvar's cross-chain sums (stats.rs:449-465) over the GATHERED per-half-chain statistics, on the device (round 5: the
 * host used to copy all N x 2 x part floats back and walk them -- 1 ms at one device, and growing with the device count):
 * block (x = 4 d + quarter, y = rank i) sums a quarter of rank i's 2 n_i half-chains of parameter d in f64 -- sum of the means,
 * of their squares, of the biased variances ssq / m -- into out[((i D + d) 4 + quarter) 3 ..]; the host adds the N x 4 partial
 * sums of a parameter in index order and forms sum((mean - overall)^2) = Sq - Sd^2 / c2.  gathered: [N][means (part) | ssq (part)],
 * a rank's valid entries first (2 n_i D), zero padding behind. */
struct GroupCounts {
    unsigned int n2[64]; /* 2 n_i; 64 entries suffice: group_create refuses more than 64 devices, so a group never has more ranks */
};
__global__ __launch_bounds__(256) void mm_group_cross_sums_kernel(const float *__restrict__ gathered, size_t part, unsigned int D,
                                                                  float nf, GroupCounts cnt, double *__restrict__ out)
{
    __shared__ double red[3][256];
    const unsigned int d = blockIdx.x >> 2, quarter = blockIdx.x & 3u, i = blockIdx.y, tid = threadIdx.x;
    const float *mi = gathered + (size_t)i * 2 * part, *qi = mi + part;
    const unsigned int c2 = cnt.n2[i], per = (c2 + 3u) / 4u, lo = quarter * per, hi = lo + per < c2 ? lo + per : c2;
    /* the means are taken relative to the mean of the FIRST half of global chain 0 -- rank 0's first entry, the very shift
     * mm_stats_tail_kernel uses on one device (means[d] of the splitcat order) -- and subtracted in f32 as there, so that
     * sum((mean - overall)^2) = Sq - Sd^2 / c2 loses no digits on a target far from the origin */
    const float shift = gathered[d];
    double sd = 0.0, sq = 0.0, ws = 0.0;
    for (unsigned int c = lo + tid; c < hi; c += 256u) {
        const double mu = (double)(mi[(size_t)c * D + d] - shift);
        sd += mu;
        sq += mu * mu;
        ws += (double)(qi[(size_t)c * D + d] / nf); /* biased per-chain variance (quirk Q8) */
    }
    red[0][tid] = sd;
    red[1][tid] = sq;
    red[2][tid] = ws;
    __syncthreads();
    for (unsigned int st = 128; st > 0; st >>= 1) {
        if (tid < st) {
            red[0][tid] += red[0][tid + st];
            red[1][tid] += red[1][tid + st];
            red[2][tid] += red[2][tid + st];
        }
        __syncthreads();
    }
    if (tid < 3)
        out[(((size_t)i * D + d) * 4 + quarter) * 3 + tid] = red[tid][0];
}

/* one host thread per device for the life of the group: calls into the per-device ABI block only their own thread,
 * and per-thread state of that ABI (the statistics' work buffers) stays with its device */
class Worker {
  public:
    Worker() : th_([this] { loop(); }) {}
    ~Worker()
    {
        {
            std::lock_guard<std::mutex> l(m_);
            quit_ = true;
        }
        cv_.notify_all();
        th_.join();
    }
    void post(std::function<int()> job)
    {
        {
            std::lock_guard<std::mutex> l(m_);
            job_ = std::move(job);
            has_job_ = true;
            done_ = false;
        }
        cv_.notify_all();
    }
    int wait()
    {
        std::unique_lock<std::mutex> l(m_);
        cv_.wait(l, [this] { return done_; });
        return rc_;
    }

  private:
    void loop()
    {
        for (;;) {
            std::function<int()> job;
            {
                std::unique_lock<std::mutex> l(m_);
                cv_.wait(l, [this] { return has_job_ || quit_; });
                if (quit_ && !has_job_)
                    return;
                job = std::move(job_);
                has_job_ = false;
            }
            const int rc = job();
            {
                std::lock_guard<std::mutex> l(m_);
                rc_ = rc;
                done_ = true;
            }
            cv_.notify_all();
        }
    }
    std::mutex m_;
    std::condition_variable cv_;
    std::function<int()> job_;
    bool has_job_ = false, done_ = true, quit_ = false;
    int rc_ = 0;
    std::thread th_;
};

struct Shard {
    int device = 0;
    size_t first = 0, n = 0; /* global chains [first, first + n) */
    void *handle = nullptr; /* the shard's sampler, of the type Group::ops drives */
    void *d_sample = nullptr; /* [n, n_collect, dim] of the last run, on the device */
    size_t sample_cap = 0;
    hipStream_t stream = nullptr;
    float *d_stats = nullptr; /* means [2 cmax, dim] | ssq [2 cmax, dim] | acov [m, dim] | gathered [N][2][2 cmax dim] */
    size_t stats_cap = 0;
    ncclComm_t comm = nullptr;
    hipEvent_t tev0 = nullptr, tev1 = nullptr; /* the stream timer (group_stream_timer) */
    std::unique_ptr<Worker> worker;
};

struct Group {
    const mm_sampler_ops *ops = nullptr; /* what differs between MH, HMC and NUTS (mm_sampler_ops.h) */
    int progress = 0; /* NUTS: run (N - 1 transitions) or run_progress stepping (nuts.rs:457-471 / 491-522) */
    int dtype = MMCMC_F32, dim = 0;
    size_t n_chains = 0, cmax = 0;
    size_t last_collect = 0;
    bool use_rccl = false, comm_ready = false;
    int exchange_status = 0; /* why the statistics travel as they do (reported through *used_rccl): mm_group_exchange's values */
    /* an asynchronous run whose enqueue loop failed half way leaves the shards at different iterations: the group refuses
     * every later run / diagnostics call with MMCMC_ERR_GROUP_BROKEN instead of continuing on an inconsistent state */
    bool broken = false;
    double phase_ms[3] = {0.0, 0.0, 0.0}; /* last group_split_rhat_ess: local partials | exchange | finish (host wall clock) */
    uint64_t user_offset = 0;
    std::vector<Shard> sh;
    size_t esize() const { return dtype == MMCMC_F32 ? 4 : 8; }
    ~Group()
    {
        /* runs may still be queued on the shards' streams (the asynchronous group_run): nothing they use may be freed under them */
        for (Shard &s : sh)
            if (s.stream && hipSetDevice(s.device) == hipSuccess)
                (void)hipStreamSynchronize(s.stream);
        for (Shard &s : sh) {
            s.worker.reset();
            (void)hipSetDevice(s.device);
            if (s.comm && rccl().ok())
                (void)rccl().CommDestroy(s.comm);
            if (s.handle)
                (void)ops->destroy(s.handle);
            if (s.d_sample)
                (void)hipFree(s.d_sample);
            if (s.d_stats)
                (void)hipFree(s.d_stats);
            if (s.tev0)
                (void)hipEventDestroy(s.tev0);
            if (s.tev1)
                (void)hipEventDestroy(s.tev1);
            if (s.stream)
                (void)hipStreamDestroy(s.stream);
        }
    }
};

template <class F> int for_each_shard(Group *g, F &&f)
{
    for (size_t i = 0; i < g->sh.size(); ++i) {
        if (!g->sh[i].worker)
            g->sh[i].worker.reset(new Worker());
        g->sh[i].worker->post([&f, g, i]() -> int { return f(g->sh[i], (int)i); });
    }
    int st = MMCMC_OK;
    for (size_t i = 0; i < g->sh.size(); ++i) {
        const int rc = g->sh[i].worker->wait();
        if (rc != MMCMC_OK && st == MMCMC_OK)
            st = rc;
    }
    return st;
}

/* H: the public handle (a Group).  make(&handle, init_slice, n, device) creates the sampler of one shard from its slice of
 * `init` [n_chains, dim] (elements of ops->init_elem_size(dtype) bytes): what a sampler's create call takes beyond that
 * stays with the mmcmc_*_group_create that passes it. */
template <class H, class Make>
int group_create(H **out, const mm_sampler_ops *ops, const mmcmc_target_desc *target, const void *init, size_t n_chains, int dtype,
                 const int *devices, int n_devices, Make &&make)
{
    if (!out)
        return MMCMC_ERR_INVALID_ARG;
    *out = nullptr;
    if (!target || !init || !devices || n_devices < 1 || n_devices > 64 || n_chains < (size_t)n_devices ||
        (dtype != MMCMC_F32 && dtype != MMCMC_F64))
        return MMCMC_ERR_INVALID_ARG;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0)
        return MMCMC_ERR_NO_DEVICE;
    for (int i = 0; i < n_devices; ++i)
        if (devices[i] < 0 || devices[i] >= n_dev)
            return MMCMC_ERR_INVALID_ARG;
    H *g = new (std::nothrow) H();
    if (!g)
        return (int)hipErrorOutOfMemory;
    g->ops = ops;
    g->dtype = dtype;
    g->dim = target->dim;
    g->n_chains = n_chains;
    const bool dup = mm_group_has_duplicate(devices, n_devices), share = dup && collectives_share_devices();
    /* the library is looked for only where the rule could use it (the first look binds it for the life of the process) */
    const mm_group_exchange_plan ex = mm_group_exchange(dup, share, mm_group_exchange(dup, share, true).use_rccl && rccl().ok());
    g->use_rccl = ex.use_rccl;
    g->exchange_status = ex.status;
    g->sh.resize((size_t)n_devices);
    g->cmax = mm_group_cmax(n_chains, (size_t)n_devices);
    for (int i = 0; i < n_devices; ++i) {
        const mm_group_slice part = mm_group_partition(n_chains, (size_t)n_devices, (size_t)i);
        g->sh[(size_t)i].device = devices[i];
        g->sh[(size_t)i].first = part.first;
        g->sh[(size_t)i].n = part.n;
    }
    const int st = for_each_shard(g, [&](Shard &s, int) -> int {
        int rc = make(&s.handle, (const char *)init + s.first * (size_t)g->dim * ops->init_elem_size(dtype), s.n, s.device);
        if (rc != MMCMC_OK)
            return rc;
        rc = ops->set_chain_offset(s.handle, s.first);
        if (rc != MMCMC_OK)
            return rc;
        if (hipSetDevice(s.device) != hipSuccess)
            return MMCMC_ERR_NO_DEVICE;
        hipError_t e = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking);
        return e == hipSuccess ? MMCMC_OK : (int)e;
    });
    if (st != MMCMC_OK) {
        delete g;
        return st;
    }
    /* the communicators are made HERE, not inside the first diagnostics call: a timed reduction never pays
     * ncclCommInitAll, and a failure is known (mmcmc_*_group_exchange) before any sampling has been paid for */
    if (g->use_rccl) {
        const size_t N = g->sh.size();
        std::vector<ncclComm_t> comms(N);
        std::vector<int> devs(N);
        for (size_t i = 0; i < N; ++i)
            devs[i] = g->sh[i].device;
        if (rccl().CommInitAll(comms.data(), (int)N, devs.data()) != 0) {
            /* e.g. no peer access: the statistics travel through the host, and the status says so */
            const mm_group_exchange_plan failed = mm_group_exchange_init_failed();
            g->use_rccl = failed.use_rccl;
            g->exchange_status = failed.status;
        } else {
            for (size_t i = 0; i < N; ++i)
                g->sh[i].comm = comms[i];
            g->comm_ready = true;
        }
    }
    *out = g;
    return MMCMC_OK;
}

/* "the same call on every shard, one after the other, stop at the first failure": the argument checks first
 * (MMCMC_ERR_INVALID_ARG), then -- for the calls that refuse a broken group, see the table above the entry points --
 * MMCMC_ERR_GROUP_BROKEN, then f(Shard &) -> status */
enum BrokenRule { kEvenIfBroken, kRefuseBroken };
template <class F> int on_every_shard(Group *g, bool args_ok, BrokenRule rule, F &&f)
{
    if (!g || !args_ok)
        return MMCMC_ERR_INVALID_ARG;
    if (rule == kRefuseBroken && g->broken)
        return MMCMC_ERR_GROUP_BROKEN;
    for (Shard &s : g->sh) {
        const int rc = f(s);
        if (rc != MMCMC_OK)
            return rc;
    }
    return MMCMC_OK;
}

int group_seed(Group *g, uint64_t seed)
{
    return on_every_shard(g, true, kEvenIfBroken, [&](Shard &s) { return g->ops->seed(s.handle, seed); });
}

int group_set_chain_offset(Group *g, uint64_t off)
{
    if (g)
        g->user_offset = off;
    return on_every_shard(g, true, kEvenIfBroken, [&](Shard &s) { return g->ops->set_chain_offset(s.handle, off + s.first); });
}

static int shard_reserve_sample(Shard &s, size_t bytes)
{
    if (bytes <= s.sample_cap)
        return MMCMC_OK;
    /* work queued on the shard's stream may still write the old buffer */
    hipError_t e = hipStreamSynchronize(s.stream);
    if (e != hipSuccess)
        return (int)e;
    if (s.d_sample)
        (void)hipFree(s.d_sample);
    s.d_sample = nullptr;
    s.sample_cap = 0;
    if ((e = hipMalloc(&s.d_sample, bytes)) != hipSuccess)
        return (int)e;
    s.sample_cap = bytes;
    return MMCMC_OK;
}

/* run(n_collect, n_discard) of every chain; the sample stays on the devices (one shard each) and, when out_host is
 * given, is also copied into the caller's [n_chains, n_collect, dim] array; accept_counts [n_chains] or NULL.  BLOCKING:
 * returns when every shard's results are there (also with out_host == NULL and accept_counts == NULL: a caller may read
 * mmcmc_*_group_shard's device pointer from any stream afterwards).  async (mmcmc_{mh,hmc}_group_run_async only):
 * enqueued on every shard's stream from this thread, returns without waiting (group_sync). */
int group_run(Group *g, size_t n_collect, size_t n_discard, void *out_host, uint64_t *accept_counts, bool async)
{
    if (!g)
        return MMCMC_ERR_INVALID_ARG;
    if (g->broken)
        return MMCMC_ERR_GROUP_BROKEN;
    const size_t esz = g->esize(), row = n_collect * (size_t)g->dim * esz;
    if (async) {
        if (!g->ops->can_run_async)
            return MMCMC_ERR_UNSUPPORTED; /* NUTS hands adaptation state over between its launches: blocking only */
        DevGuard restore; /* the loops below set each shard's device */
        int st = MMCMC_OK;
        /* every allocation first: a failure here has advanced no shard */
        for (Shard &s : g->sh) {
            if (hipSetDevice(s.device) != hipSuccess) {
                st = MMCMC_ERR_NO_DEVICE;
                break;
            }
            if ((st = shard_reserve_sample(s, s.n * row)) != MMCMC_OK)
                break;
        }
        size_t enqueued = 0;
        if (st == MMCMC_OK)
            for (Shard &s : g->sh) {
                if (hipSetDevice(s.device) != hipSuccess) {
                    st = MMCMC_ERR_NO_DEVICE;
                    break;
                }
                st = g->ops->run(s.handle, n_collect, n_discard, n_collect ? s.d_sample : nullptr, nullptr, 0, s.stream);
                if (st != MMCMC_OK)
                    break;
                ++enqueued;
            }
        if (mm_group_breaks_async(enqueued, st)) {
            /* shards 0 .. enqueued - 1 have advanced, the rest have not: wait for what was queued and refuse further use */
            for (size_t i = 0; i < enqueued; ++i)
                if (hipSetDevice(g->sh[i].device) == hipSuccess)
                    (void)hipStreamSynchronize(g->sh[i].stream);
            g->broken = true;
        }
        if (st == MMCMC_OK)
            g->last_collect = n_collect;
        return st;
    }
    std::vector<char> advanced(g->sh.size(), 0); /* which shards' samplers have run (each written by its own worker) */
    const int st = for_each_shard(g, [&](Shard &s, int i) -> int {
        if (hipSetDevice(s.device) != hipSuccess)
            return MMCMC_ERR_NO_DEVICE;
        const size_t bytes = s.n * row;
        int rc = shard_reserve_sample(s, bytes);
        if (rc != MMCMC_OK)
            return rc;
        uint64_t *acc = accept_counts ? accept_counts + s.first : nullptr;
        rc = g->ops->run(s.handle, n_collect, n_discard, n_collect ? s.d_sample : nullptr, acc, g->progress, s.stream);
        if (rc != MMCMC_OK)
            return rc;
        advanced[(size_t)i] = 1;
        hipError_t e = hipSuccess;
        if (out_host && n_collect) /* through the device's own pinned bounce ring: every shard over its own link, side by side */
            e = mm_copy_to_host((char *)out_host + s.first * row, s.d_sample, bytes, s.device, s.stream);
        else
            e = hipStreamSynchronize(s.stream);
        return e == hipSuccess ? MMCMC_OK : (int)e;
    });
    /* when every shard ran but a copy or sync failed, last_collect keeps the length of the run before (kept as it is) */
    if (st == MMCMC_OK)
        g->last_collect = n_collect;
    size_t n_adv = 0;
    for (char a : advanced)
        n_adv += a ? 1 : 0;
    if (mm_group_breaks_blocking(n_adv, g->sh.size(), st))
        g->broken = true; /* some shards have run and others not: same rule as the asynchronous path */
    return st;
}

/* wait for everything queued on the shards' streams */
int group_sync(Group *g)
{
    if (!g)
        return MMCMC_ERR_INVALID_ARG;
    DevGuard restore;
    int st = MMCMC_OK;
    for (Shard &s : g->sh) {
        hipError_t e = hipSetDevice(s.device);
        if (e == hipSuccess)
            e = hipStreamSynchronize(s.stream);
        if (e != hipSuccess && st == MMCMC_OK)
            st = (int)e;
    }
    return st;
}

/* Stream timer: stop = 0 records a start event on every shard's stream; stop = 1 records the end events, waits for them
 * and writes the elapsed milliseconds of every shard into ms [n_devices] -- the time the DEVICE spent on what was queued
 * in between (bench.py: kernel time per device of a scaling run, free of the host's launch loop). */
int group_stream_timer(Group *g, int stop, float *ms)
{
    if (!g || (stop && !ms))
        return MMCMC_ERR_INVALID_ARG;
    DevGuard restore;
    hipError_t e = hipSuccess;
    for (Shard &s : g->sh) {
        if ((e = hipSetDevice(s.device)) != hipSuccess)
            break;
        if (!s.tev0 && (e = hipEventCreate(&s.tev0)) != hipSuccess)
            break;
        if (!s.tev1 && (e = hipEventCreate(&s.tev1)) != hipSuccess)
            break;
        if ((e = hipEventRecord(stop ? s.tev1 : s.tev0, s.stream)) != hipSuccess)
            break;
    }
    if (e == hipSuccess && stop) {
        size_t i = 0;
        for (Shard &s : g->sh) {
            if ((e = hipSetDevice(s.device)) != hipSuccess || (e = hipEventSynchronize(s.tev1)) != hipSuccess ||
                (e = hipEventElapsedTime(&ms[i], s.tev0, s.tev1)) != hipSuccess)
                break;
            ++i;
        }
    }
    return e == hipSuccess ? MMCMC_OK : (int)e;
}

/* how the diagnostics' statistics will travel (decided at creation): the values of *used_rccl */
int group_exchange(Group *g, int *status, int *n_rccl_ranks)
{
    if (!g || !status)
        return MMCMC_ERR_INVALID_ARG;
    *status = g->exchange_status;
    if (n_rccl_ranks)
        *n_rccl_ranks = g->comm_ready ? (int)g->sh.size() : 0;
    return MMCMC_OK;
}

int group_state(Group *g, void *out)
{
    if (!g || !out)
        return MMCMC_ERR_INVALID_ARG;
    /* a broken group's shards stand at different iterations; their states are still what each shard holds -- readable */
    const size_t esz = g->esize();
    return for_each_shard(g, [&](Shard &s, int) -> int {
        return g->ops->state(s.handle, (char *)out + s.first * (size_t)g->dim * esz);
    });
}

/* positions [n_chains, dim] (host; NUTS: of the tensor type) split across the shards; each copy is ordered behind the
 * runs queued on its shard's stream and done when the call returns */
int group_set_state(Group *g, const void *in)
{
    if (!g || !in)
        return MMCMC_ERR_INVALID_ARG;
    if (g->broken)
        return MMCMC_ERR_GROUP_BROKEN;
    const size_t esz = g->esize();
    return for_each_shard(g, [&](Shard &s, int) -> int {
        return g->ops->set_state(s.handle, (const char *)in + s.first * (size_t)g->dim * esz, s.stream);
    });
}

/* (seed, first global chain, iteration): the shards share seed and iteration; their chain offsets follow from the first */
int group_stream_position(Group *g, uint64_t *seed, uint64_t *first_global_chain, uint64_t *iteration)
{
    if (!g)
        return MMCMC_ERR_INVALID_ARG;
    if (g->broken)
        return MMCMC_ERR_GROUP_BROKEN; /* the shards stand at different iterations */
    const int rc = g->ops->stream_position(g->sh[0].handle, seed, nullptr, iteration);
    if (rc == MMCMC_OK && first_global_chain)
        *first_global_chain = g->user_offset;
    return rc;
}

int group_set_iteration(Group *g, uint64_t iteration)
{
    return on_every_shard(g, iteration < (1ull << 32), kRefuseBroken, [&](Shard &s) { return g->ops->set_iteration(s.handle, iteration); });
}

/* split-R-hat / ESS of the last run's sample (stats.rs:416-423) over ALL devices' chains */
int group_split_rhat_ess(Group *g, float *rhat, float *ess, int *used_rccl)
{
    if (!g || !rhat || !ess)
        return MMCMC_ERR_INVALID_ARG;
    if (g->broken)
        return MMCMC_ERR_GROUP_BROKEN;
    const size_t n = g->last_collect, m = n / 2, D = (size_t)g->dim, N = g->sh.size();
    if (m < 1)
        return MMCMC_ERR_SHAPE;
    using clk = std::chrono::steady_clock;
    const clk::time_point t_begin = clk::now();
    clk::time_point t_local = t_begin, t_exch = t_begin;
    auto phases = [&](int rc) { /* local partials | exchange (collectives + cross sums / host copies) | finish */
        const clk::time_point t_end = clk::now();
        g->phase_ms[0] = std::chrono::duration<double, std::milli>(t_local - t_begin).count();
        g->phase_ms[1] = std::chrono::duration<double, std::milli>(t_exch - t_local).count();
        g->phase_ms[2] = std::chrono::duration<double, std::milli>(t_end - t_exch).count();
        return rc;
    };
    const size_t part = 2 * g->cmax * D;             /* per-device means (or ssq), padded to the largest shard */
    const size_t own = 2 * part + m * D;             /* means | ssq | acov */
    const size_t n_cs = N * D * 4 * 3;               /* partial cross-chain sums (f64) of mm_group_cross_sums_kernel */
    const size_t total = own + N * 2 * part + m * D + 2 * n_cs + 2; /* + gathered [N][means | ssq] + reduced acov + the partial sums */
    if (used_rccl)
        *used_rccl = g->exchange_status;
    std::vector<float> h_own(g->use_rccl ? 0 : N * own);
    /* phase 1: every shard's local statistics, finished and checked BEFORE any rank enters a collective -- a shard that
     * failed here would otherwise leave the others waiting in ncclAllGather for good */
    int st = for_each_shard(g, [&](Shard &s, int) -> int {
        if (hipSetDevice(s.device) != hipSuccess)
            return MMCMC_ERR_NO_DEVICE;
        hipError_t e;
        if (total > s.stats_cap) {
            if (s.d_stats)
                (void)hipFree(s.d_stats);
            s.d_stats = nullptr;
            s.stats_cap = 0;
            if ((e = hipMalloc((void **)&s.d_stats, total * sizeof(float))) != hipSuccess)
                return (int)e;
            s.stats_cap = total;
        }
        float *means = s.d_stats, *ssq = means + part, *acov = ssq + part;
        if ((e = hipMemsetAsync(s.d_stats, 0, own * sizeof(float), s.stream)) != hipSuccess)
            return (int)e;
        /* the local statistics are [2][n_i][D] (first halves of the local chains, then their second halves); every
         * rank sends a slot of 2 * cmax * D floats (all-gather wants equal counts), the tail past 2 n_i D stays zero */
        int rc = mmcmc_stats_partials(s.d_sample, g->dtype, s.n, n, D, means, ssq, acov, s.device, s.stream);
        if (rc != MMCMC_OK)
            return rc;
        e = hipStreamSynchronize(s.stream);
        return e == hipSuccess ? MMCMC_OK : (int)e;
    });
    if (st != MMCMC_OK)
        return st;
    t_local = t_exch = clk::now();
    /* phase 2: the exchange */
    st = for_each_shard(g, [&](Shard &s, int i) -> int {
        if (hipSetDevice(s.device) != hipSuccess)
            return MMCMC_ERR_NO_DEVICE;
        hipError_t e;
        float *means = s.d_stats, *ssq = means + part, *acov = ssq + part, *gathered = acov + m * D, *acov_all = gathered + N * 2 * part;
        (void)ssq;
        if (g->use_rccl) {
            /* means and ssq are adjacent: one all-gather of 2 * part floats per rank; lag sums: one all-reduce */
            if (rccl().AllGather(means, gathered, 2 * part, kNcclFloat32, s.comm, s.stream) != 0)
                return (int)hipErrorUnknown;
            if (rccl().AllReduce(acov, acov_all, m * D, kNcclFloat32, kNcclSum, s.comm, s.stream) != 0)
                return (int)hipErrorUnknown;
            if (i == 0) { /* the cross-chain sums of ALL ranks' half-chains, from shard 0's copy of the gathered statistics */
                GroupCounts cnt;
                for (size_t r = 0; r < N; ++r)
                    cnt.n2[r] = (unsigned int)(2 * g->sh[r].n);
                double *cs = reinterpret_cast<double *>(s.d_stats + ((own + N * 2 * part + m * D + 1) / 2) * 2);
                hipLaunchKernelGGL(mm_group_cross_sums_kernel, dim3((unsigned int)D * 4u, (unsigned int)N), dim3(256), 0, s.stream, gathered,
                                   part, (unsigned int)D, (float)m, cnt, cs);
                if ((e = hipGetLastError()) != hipSuccess)
                    return (int)e;
            }
        } else {
            if ((e = hipMemcpyAsync(h_own.data() + (size_t)i * own, s.d_stats, own * sizeof(float), hipMemcpyDeviceToHost, s.stream)) != hipSuccess)
                return (int)e;
        }
        e = hipStreamSynchronize(s.stream);
        return e == hipSuccess ? MMCMC_OK : (int)e;
    });
    if (st != MMCMC_OK)
        return st;
    t_exch = clk::now();
    /* RCCL path: the finish needs the gathered statistics only through their cross-chain sums, which shard 0 has reduced on
     * the device.  Host-exchange path (a device listed twice, no RCCL): the host walks the statistics in splitcat order (first
     * halves of all chains, then second halves) */
    std::vector<float> acov;
    if (g->use_rccl) {
        /* a few KB come back: the reduced lag sums and the N x 4 partial cross-chain sums per parameter */
        Shard &s0 = g->sh[0];
        (void)hipSetDevice(s0.device);
        const float *acov_all = s0.d_stats + own + N * 2 * part;
        const double *cs = reinterpret_cast<const double *>(s0.d_stats + ((own + N * 2 * part + m * D + 1) / 2) * 2);
        std::vector<double> h_cs(n_cs);
        acov.resize(m * D);
        hipError_t e = hipMemcpy(acov.data(), acov_all, acov.size() * sizeof(float), hipMemcpyDeviceToHost);
        if (e == hipSuccess)
            e = hipMemcpy(h_cs.data(), cs, n_cs * sizeof(double), hipMemcpyDeviceToHost);
        if (e != hipSuccess)
            return (int)e;
        const double c2 = 2.0 * (double)g->n_chains;
        std::vector<double> dsum(D), wsum(D);
        for (size_t d = 0; d < D; ++d) {
            double sd = 0.0, sq = 0.0, ws = 0.0;
            for (size_t r = 0; r < N; ++r)
                for (size_t qtr = 0; qtr < 4; ++qtr) {
                    const double *q3 = h_cs.data() + ((r * D + d) * 4 + qtr) * 3;
                    sd += q3[0];
                    sq += q3[1];
                    ws += q3[2];
                }
            const double ds = sq - sd * sd / c2; /* sum of (mean - overall mean)^2 */
            dsum[d] = ds > 0.0 ? ds : 0.0;
            wsum[d] = ws;
        }
        return phases(mmcmc_stats_finish_sums(dsum.data(), wsum.data(), acov.data(), 2 * g->n_chains, m, D, rhat, ess));
    }
    std::vector<float> g_all(N * 2 * part);
    acov.assign(m * D, 0.f);
    for (size_t i = 0; i < N; ++i) {
        std::memcpy(g_all.data() + i * 2 * part, h_own.data() + i * own, 2 * part * sizeof(float));
        const float *a = h_own.data() + i * own + 2 * part;
        for (size_t k = 0; k < m * D; ++k)
            acov[k] += a[k];
    }
    const size_t C = g->n_chains;
    std::vector<float> means(2 * C * D), ssq(2 * C * D);
    for (size_t i = 0; i < N; ++i) {
        const Shard &s = g->sh[i];
        const float *mi = g_all.data() + i * 2 * part, *qi = mi + part;
        for (int half = 0; half < 2; ++half) {
            std::memcpy(means.data() + ((size_t)half * C + s.first) * D, mi + (size_t)half * s.n * D, s.n * D * sizeof(float));
            std::memcpy(ssq.data() + ((size_t)half * C + s.first) * D, qi + (size_t)half * s.n * D, s.n * D * sizeof(float));
        }
    }
    return phases(mmcmc_stats_finish(means.data(), ssq.data(), acov.data(), 2 * C, m, D, rhat, ess));
}

int group_stats_phases(Group *g, double *ms3)
{
    if (!g || !ms3)
        return MMCMC_ERR_INVALID_ARG;
    for (int i = 0; i < 3; ++i)
        ms3[i] = g->phase_ms[i];
    return MMCMC_OK;
}

/* the typed calls only one sampler has (its fields, NUTS's adaptation records) take the shard's handle through these */
mmcmc_mh *mh_of(const Shard &s) { return (mmcmc_mh *)s.handle; }
mmcmc_hmc *hmc_of(const Shard &s) { return (mmcmc_hmc *)s.handle; }
mmcmc_nuts *nuts_of(const Shard &s) { return (mmcmc_nuts *)s.handle; }

} // namespace

/* the public handles are the group */
struct mmcmc_mh_group : Group {};
struct mmcmc_hmc_group : Group {};
struct mmcmc_nuts_group : Group {};

/* Every entry point checks a NULL handle and its arguments first (MMCMC_ERR_INVALID_ARG).  Then:
 *
 *   refuse a broken group (MMCMC_ERR_GROUP_BROKEN)      | do not look at `broken`
 *   ----------------------------------------------------+------------------------------------------------------------
 *   run, run_async                                      | seed, set_chain_offset, set_max_depth (*)
 *   set_state, stream_position, set_iteration           | state, adapt_state, leapfrog_counts, *_params, shard
 *   split_rhat_mean_ess                                 | sync, stream_timer, exchange, stats_phases, destroy
 *   set_step_size, set_n_leapfrog, set_proposal_std,    | set_draw_stats (always MMCMC_ERR_UNSUPPORTED)
 *   set_target_accept_p, set_adapt_state                |
 *
 * (*) the odd one out among the setters: observed, not decided. */
extern "C" {

int mmcmc_group_bind_collectives(const char *library_path, int ranks_may_share_a_device)
{
    return bind_collectives(library_path, ranks_may_share_a_device);
}

/* what all three samplers' groups have */
#define MM_GROUP_COMMON(P)                                                                                        \
    int mmcmc_##P##_group_seed(mmcmc_##P##_group *h, uint64_t seed) { return group_seed(h, seed); }               \
    int mmcmc_##P##_group_set_chain_offset(mmcmc_##P##_group *h, uint64_t off) { return group_set_chain_offset(h, off); } \
    int mmcmc_##P##_group_stats_phases(mmcmc_##P##_group *h, double *ms3) { return group_stats_phases(h, ms3); }  \
    int mmcmc_##P##_group_state(mmcmc_##P##_group *h, void *out) { return group_state(h, out); }                  \
    int mmcmc_##P##_group_set_state(mmcmc_##P##_group *h, const void *in) { return group_set_state(h, in); }      \
    int mmcmc_##P##_group_stream_position(mmcmc_##P##_group *h, uint64_t *seed, uint64_t *first_global_chain, uint64_t *iteration) \
    {                                                                                                             \
        return group_stream_position(h, seed, first_global_chain, iteration);                                     \
    }                                                                                                             \
    int mmcmc_##P##_group_set_iteration(mmcmc_##P##_group *h, uint64_t iteration) { return group_set_iteration(h, iteration); } \
    int mmcmc_##P##_group_split_rhat_mean_ess(mmcmc_##P##_group *h, float *rhat, float *ess, int *used_rccl)      \
    {                                                                                                             \
        return group_split_rhat_ess(h, rhat, ess, used_rccl);                                                     \
    }                                                                                                             \
    int mmcmc_##P##_group_sync(mmcmc_##P##_group *h) { return group_sync(h); }                                    \
    int mmcmc_##P##_group_stream_timer(mmcmc_##P##_group *h, int stop, float *ms_per_device)                      \
    {                                                                                                             \
        return group_stream_timer(h, stop, ms_per_device);                                                        \
    }                                                                                                             \
    int mmcmc_##P##_group_exchange(mmcmc_##P##_group *h, int *status, int *n_rccl_ranks)                          \
    {                                                                                                             \
        return group_exchange(h, status, n_rccl_ranks);                                                           \
    }                                                                                                             \
    int mmcmc_##P##_group_destroy(mmcmc_##P##_group *h)                                                         \
    {                                                                                                             \
        delete h; /* ~Group */                                                                                    \
        return h ? MMCMC_OK : MMCMC_ERR_INVALID_ARG;                                                              \
    }
MM_GROUP_COMMON(mh)
MM_GROUP_COMMON(hmc)
MM_GROUP_COMMON(nuts)
#undef MM_GROUP_COMMON

/* ---- HMC ---- */
int mmcmc_hmc_group_create(mmcmc_hmc_group **out, const mmcmc_target_desc *target, const void *init, size_t n_chains,
                           double step_size, int n_leapfrog, int dtype, const int *devices, int n_devices)
{
    return group_create(out, &mm_ops_hmc, target, init, n_chains, dtype, devices, n_devices,
                        [&](void **handle, const void *x, size_t n, int device) -> int {
                            mmcmc_hmc *h = nullptr;
                            const int rc = mmcmc_hmc_create(&h, target, x, n, step_size, n_leapfrog, dtype, device);
                            /* nobody reads the per-handle launch timing of a shard: no event packets between back-to-back launches */
                            if (rc == MMCMC_OK)
                                (void)mmcmc_hmc_enable_timing(h, 0);
                            *handle = h;
                            return rc;
                        });
}
int mmcmc_hmc_group_run(mmcmc_hmc_group *h, size_t n_collect, size_t n_discard, void *out_host, uint64_t *accept_counts)
{
    return group_run(h, n_collect, n_discard, out_host, accept_counts, false);
}
int mmcmc_hmc_group_run_async(mmcmc_hmc_group *h, size_t n_collect, size_t n_discard)
{
    return group_run(h, n_collect, n_discard, nullptr, nullptr, true);
}
int mmcmc_hmc_group_set_step_size(mmcmc_hmc_group *h, double step_size)
{
    /* checked once, here: no shard changes unless all do */
    return on_every_shard(h, step_size > 0.0 && std::isfinite(step_size), kRefuseBroken,
                          [&](Shard &s) { return mmcmc_hmc_set_step_size(hmc_of(s), step_size); });
}
int mmcmc_hmc_group_set_n_leapfrog(mmcmc_hmc_group *h, int n_leapfrog)
{
    return on_every_shard(h, n_leapfrog >= 0, kRefuseBroken, [&](Shard &s) { return mmcmc_hmc_set_n_leapfrog(hmc_of(s), n_leapfrog); });
}
int mmcmc_hmc_group_params(mmcmc_hmc_group *h, double *step_size, int *n_leapfrog)
{
    return h ? mmcmc_hmc_params(hmc_of(h->sh[0]), step_size, n_leapfrog) : MMCMC_ERR_INVALID_ARG;
}
int mmcmc_hmc_group_shard(mmcmc_hmc_group *h, int i, int *device, size_t *first_chain, size_t *n_chains, void **sample_dev)
{
    if (!h || i < 0 || (size_t)i >= h->sh.size())
        return MMCMC_ERR_INVALID_ARG;
    const Shard &s = h->sh[(size_t)i];
    if (device)
        *device = s.device;
    if (first_chain)
        *first_chain = s.first;
    if (n_chains)
        *n_chains = s.n;
    if (sample_dev)
        *sample_dev = s.d_sample;
    return MMCMC_OK;
}

/* ---- MH ---- */
int mmcmc_mh_group_create(mmcmc_mh_group **out, const mmcmc_target_desc *target, const mmcmc_proposal_desc *proposal,
                          const void *init, size_t n_chains, int dtype, const int *devices, int n_devices)
{
    if (!out || !proposal) /* before anything else */
        return MMCMC_ERR_INVALID_ARG;
    return group_create(out, &mm_ops_mh, target, init, n_chains, dtype, devices, n_devices,
                        [&](void **handle, const void *x, size_t n, int device) -> int {
                            mmcmc_mh *h = nullptr;
                            const int rc = mmcmc_mh_create(&h, target, proposal, x, n, dtype, device);
                            if (rc == MMCMC_OK) /* as for HMC */
                                (void)mmcmc_mh_enable_timing(h, 0);
                            *handle = h;
                            return rc;
                        });
}
int mmcmc_mh_group_run(mmcmc_mh_group *h, size_t n_collect, size_t n_discard, void *out_host, uint64_t *accept_counts)
{
    return group_run(h, n_collect, n_discard, out_host, accept_counts, false);
}
int mmcmc_mh_group_run_async(mmcmc_mh_group *h, size_t n_collect, size_t n_discard)
{
    return group_run(h, n_collect, n_discard, nullptr, nullptr, true);
}
int mmcmc_mh_group_set_proposal_std(mmcmc_mh_group *h, double std)
{
    return on_every_shard(h, std > 0.0 && std::isfinite(std), kRefuseBroken, [&](Shard &s) { return mmcmc_mh_set_proposal_std(mh_of(s), std); });
}
int mmcmc_mh_group_params(mmcmc_mh_group *h, double *std) { return h ? mmcmc_mh_params(mh_of(h->sh[0]), std) : MMCMC_ERR_INVALID_ARG; }

/* ---- NUTS::run / run_progress (nuts.rs:163-170, 194-338) over N devices: `init` [n_chains, dim] doubles, mode as in
 * mmcmc_nuts_create; the sample is of the mode's tensor type (f32 for modes 0 and 1, f64 for mode 2) ---- */
int mmcmc_nuts_group_create(mmcmc_nuts_group **out, const mmcmc_target_desc *target, const double *init, size_t n_chains,
                            double target_accept_p, int mode, const int *devices, int n_devices)
{
    if (!out || mode < 0 || mode > 2)
        return MMCMC_ERR_INVALID_ARG;
    return group_create(out, &mm_ops_nuts, target, init, n_chains, mode == 2 ? MMCMC_F64 : MMCMC_F32, devices, n_devices,
                        [&](void **handle, const void *x, size_t n, int device) -> int {
                            mmcmc_nuts *h = nullptr;
                            const int rc = mmcmc_nuts_create(&h, target, (const double *)x, n, target_accept_p, mode, device);
                            *handle = h;
                            return rc;
                        });
}
int mmcmc_nuts_group_run(mmcmc_nuts_group *h, size_t n_collect, size_t n_discard, void *out_host, int progress)
{
    if (!h)
        return MMCMC_ERR_INVALID_ARG;
    h->progress = progress ? 1 : 0; /* run (N - 1 transitions) or run_progress stepping (nuts.rs:457-471 / 491-522) */
    return group_run(h, n_collect, n_discard, out_host, nullptr, false);
}
int mmcmc_nuts_group_set_max_depth(mmcmc_nuts_group *h, int max_depth)
{
    /* the range is the shard's check (mmcmc_nuts_set_max_depth); a broken group is not refused: see the table */
    return on_every_shard(h, true, kEvenIfBroken, [&](Shard &s) { return mmcmc_nuts_set_max_depth(nuts_of(s), max_depth); });
}
int mmcmc_nuts_group_set_target_accept_p(mmcmc_nuts_group *h, double target_accept_p)
{
    return on_every_shard(h, target_accept_p > 0.0 && target_accept_p < 1.0, kRefuseBroken,
                          [&](Shard &s) { return mmcmc_nuts_set_target_accept_p(nuts_of(s), target_accept_p); });
}
int mmcmc_nuts_group_params(mmcmc_nuts_group *h, double *target_accept_p, int *max_depth)
{
    return h ? mmcmc_nuts_params(nuts_of(h->sh[0]), target_accept_p, max_depth) : MMCMC_ERR_INVALID_ARG;
}
/* per-draw statistics (mmcmc_nuts_set_draw_stats) are a single handle's: a device group does not record, and nothing changes */
int mmcmc_nuts_group_set_draw_stats(mmcmc_nuts_group *h, int) { return h ? MMCMC_ERR_UNSUPPORTED : MMCMC_ERR_INVALID_ARG; }
int mmcmc_nuts_group_leapfrog_counts(mmcmc_nuts_group *h, uint64_t *out)
{
    if (!h || !out)
        return MMCMC_ERR_INVALID_ARG;
    return for_each_shard(h, [&](Shard &s, int) -> int { return mmcmc_nuts_leapfrog_counts(nuts_of(s), out + s.first); });
}
int mmcmc_nuts_group_adapt_state(mmcmc_nuts_group *h, double *out)
{
    if (!h || !out)
        return MMCMC_ERR_INVALID_ARG;
    return for_each_shard(h, [&](Shard &s, int) -> int { return mmcmc_nuts_adapt_state(nuts_of(s), out + 4 * s.first); });
}
int mmcmc_nuts_group_set_adapt_state(mmcmc_nuts_group *h, const double *in)
{
    if (!h || !in)
        return MMCMC_ERR_INVALID_ARG;
    if (h->broken)
        return MMCMC_ERR_GROUP_BROKEN;
    /* mmcmc_nuts_set_adapt_state's checks on every row first: no shard changes unless all do */
    int mode = 0;
    (void)mmcmc_nuts_shape(nuts_of(h->sh[0]), nullptr, nullptr, &mode, nullptr);
    for (size_t i = 0; i < 4 * h->n_chains; ++i) {
        const double v = in[i];
        if (!std::isfinite(v) || (mode == 1 && !std::isfinite((float)v)))
            return MMCMC_ERR_INVALID_ARG;
        if (i % 4 == 0 && !((mode == 1 ? (double)(float)v : v) > 0.0) && v != -1.0)
            return MMCMC_ERR_INVALID_ARG;
    }
    return for_each_shard(h, [&](Shard &s, int) -> int { return mmcmc_nuts_set_adapt_state(nuts_of(s), in + 4 * s.first); });
}

} /* extern "C" */
