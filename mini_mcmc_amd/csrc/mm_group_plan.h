/* mm_group_plan.h -- the host rules a device group (mm_group.hip) runs on: which chains go to which shard, how the
 * diagnostics' statistics travel, and when a failed run leaves the group broken.  Pure host functions; no HIP include, so
 * tests/cpp/group_plan.cpp walks them with a plain C++17 compiler.  Internal linkage: nothing here joins the library's
 * exported symbols. */
#ifndef MM_GROUP_PLAN_H
#define MM_GROUP_PLAN_H

#include "../../include/mmcmc.h"

/* shard i of n_devices holds the global chains [first, first + n): contiguous blocks, the n_chains % n_devices larger
 * ones (one chain more) first */
struct mm_group_slice {
    size_t first, n;
};
static inline mm_group_slice mm_group_partition(size_t n_chains, size_t n_devices, size_t i)
{
    const size_t base = n_chains / n_devices, rem = n_chains % n_devices;
    return {i * base + (i < rem ? i : rem), base + (i < rem ? 1 : 0)};
}
/* the largest shard: what every rank's slot of the gathered statistics is padded to */
static inline size_t mm_group_cmax(size_t n_chains, size_t n_devices) { return mm_group_partition(n_chains, n_devices, 0).n; }

static inline bool mm_group_has_duplicate(const int *devices, int n)
{
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j)
            if (devices[j] == devices[i])
                return true;
    return false;
}

/* How the statistics travel, and the status reported through *used_rccl / mmcmc_*_group_exchange:
 *    1  the collectives;
 *    0  the host BY DESIGN: a device listed twice, and the library does not take two ranks on one device (RCCL does not);
 *   -1  the host as a FALLBACK: no collective library found;
 *   -2  the host as a FALLBACK: ncclCommInitAll failed (e.g. no peer access)
 * -- a scaling run must not take the host path silently. */
struct mm_group_exchange_plan {
    bool use_rccl;
    int status;
};
static inline mm_group_exchange_plan mm_group_exchange(bool dup, bool share_devices, bool collectives_ok)
{
    const bool use = (!dup || share_devices) && collectives_ok;
    return {use, use ? 1 : dup ? 0 : -1};
}
static inline mm_group_exchange_plan mm_group_exchange_init_failed() { return {false, -2}; }

/* A failed run that leaves the shards at different iterations breaks the group (MMCMC_ERR_GROUP_BROKEN from then on).
 * Blocking: every shard runs on its own thread, so "some but not all have advanced".  Asynchronous: the shards are
 * enqueued in order and the loop stops at the first failure, so "at least one was enqueued". */
static inline bool mm_group_breaks_blocking(size_t n_advanced, size_t n_shards, int status)
{
    return status != MMCMC_OK && n_advanced > 0 && n_advanced < n_shards;
}
static inline bool mm_group_breaks_async(size_t n_enqueued, int status) { return status != MMCMC_OK && n_enqueued > 0; }

#endif
