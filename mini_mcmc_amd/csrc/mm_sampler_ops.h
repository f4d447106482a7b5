/* mm_sampler_ops.h -- what differs between MH, HMC and NUTS for code that drives a handle from outside (the device groups
 * of mm_group.hip, the progress runners of mm_progress.hip): one table of function pointers over a `void *` handle and
 * three constant instances.  The members are the calls those two units make, nothing else; creation is not among them
 * (the argument lists differ: each mmcmc_*_group_create brings its own).  Host code over the public C ABI; internal
 * linkage, so nothing here joins the library's exported symbols. */
#ifndef MM_SAMPLER_OPS_H
#define MM_SAMPLER_OPS_H

#include "../../include/mmcmc.h"

struct mm_sampler_ops {
    int (*destroy)(void *h);
    int (*seed)(void *h, uint64_t seed);
    int (*set_chain_offset)(void *h, uint64_t first_global_chain);
    /* run(n_collect, n_discard) into DEVICE memory d_out [n_chains, n_collect, dim] (NULL: no sample).  accept_counts (host
     * [n_chains] or NULL): MH and HMC; progress (mmcmc_nuts_run's): NUTS.  Each sampler ignores what it does not take. */
    int (*run)(void *h, size_t n_collect, size_t n_discard, void *d_out, uint64_t *accept_counts, int progress, void *stream);
    int (*state)(void *h, void *out_host);
    int (*set_state)(void *h, const void *in_host, void *stream);
    int (*stream_position)(void *h, uint64_t *seed, uint64_t *chain_offset, uint64_t *iteration);
    int (*set_iteration)(void *h, uint64_t iteration);
    /* rows [row0, row0 + n_rows) of a device sample [n_chains, n_total_rows, dim]; NUTS has no such call: null */
    int (*run_rows)(void *h, size_t n_rows, size_t n_discard, void *out_device, size_t n_total_rows, size_t row0, void *stream);
    bool per_chain_trackers; /* run_progress: ChainTrackers through the burn-in (MH, NUTS); HMC: one MultiChainTracker after it */
    bool can_run_async;      /* a run is one enqueue; NUTS hands adaptation state over between its launches: blocking only */
    size_t (*init_elem_size)(int dtype); /* of the initial positions a create call takes: NUTS always doubles (nuts.rs:123-129) */
};

#define MM_SAMPLER_ADAPTERS(P)                                                                                    \
    static int mm_##P##_destroy(void *h) { return mmcmc_##P##_destroy((mmcmc_##P *)h); }                          \
    static int mm_##P##_seed(void *h, uint64_t seed) { return mmcmc_##P##_seed((mmcmc_##P *)h, seed); }           \
    static int mm_##P##_set_chain_offset(void *h, uint64_t off) { return mmcmc_##P##_set_chain_offset((mmcmc_##P *)h, off); } \
    static int mm_##P##_state(void *h, void *out) { return mmcmc_##P##_state((mmcmc_##P *)h, out); }              \
    static int mm_##P##_set_state(void *h, const void *in, void *stream) { return mmcmc_##P##_set_state((mmcmc_##P *)h, in, 0, stream); } \
    static int mm_##P##_stream_position(void *h, uint64_t *seed, uint64_t *off, uint64_t *it)                     \
    {                                                                                                             \
        return mmcmc_##P##_stream_position((mmcmc_##P *)h, seed, off, it);                                        \
    }                                                                                                             \
    static int mm_##P##_set_iteration(void *h, uint64_t it) { return mmcmc_##P##_set_iteration((mmcmc_##P *)h, it); }
/* the two fixed-length samplers: accept counts, and a run into some rows of a larger sample */
#define MM_FIXED_ADAPTERS(P)                                                                                      \
    MM_SAMPLER_ADAPTERS(P)                                                                                        \
    static int mm_##P##_run(void *h, size_t n_collect, size_t n_discard, void *d_out, uint64_t *acc, int, void *stream) \
    {                                                                                                             \
        return mmcmc_##P##_run((mmcmc_##P *)h, n_collect, n_discard, d_out, 1, acc, stream);                      \
    }                                                                                                             \
    static int mm_##P##_rows(void *h, size_t n_rows, size_t n_discard, void *out, size_t n_total, size_t row0, void *stream) \
    {                                                                                                             \
        return mmcmc_##P##_run_rows((mmcmc_##P *)h, n_rows, n_discard, out, n_total, row0, stream);               \
    }
#define MM_SAMPLER_OPS(P, ROWS, PER_CHAIN, ASYNC, ESIZE)                                                          \
    {mm_##P##_destroy, mm_##P##_seed, mm_##P##_set_chain_offset, mm_##P##_run, mm_##P##_state, mm_##P##_set_state, \
     mm_##P##_stream_position, mm_##P##_set_iteration, ROWS, PER_CHAIN, ASYNC, ESIZE}

MM_FIXED_ADAPTERS(mh)
MM_FIXED_ADAPTERS(hmc)
MM_SAMPLER_ADAPTERS(nuts)
static int mm_nuts_run(void *h, size_t n_collect, size_t n_discard, void *d_out, uint64_t *, int progress, void *stream)
{
    return mmcmc_nuts_run((mmcmc_nuts *)h, n_collect, n_discard, d_out, 1, progress, stream);
}
static size_t mm_esize_of_dtype(int dtype) { return dtype == MMCMC_F32 ? 4 : 8; }
static size_t mm_esize_double(int) { return sizeof(double); }

static const mm_sampler_ops mm_ops_mh = MM_SAMPLER_OPS(mh, mm_mh_rows, true, true, mm_esize_of_dtype);
static const mm_sampler_ops mm_ops_hmc = MM_SAMPLER_OPS(hmc, mm_hmc_rows, false, true, mm_esize_of_dtype);
static const mm_sampler_ops mm_ops_nuts = MM_SAMPLER_OPS(nuts, nullptr, true, false, mm_esize_double);

#undef MM_SAMPLER_ADAPTERS
#undef MM_FIXED_ADAPTERS
#undef MM_SAMPLER_OPS

#endif /* MM_SAMPLER_OPS_H */
