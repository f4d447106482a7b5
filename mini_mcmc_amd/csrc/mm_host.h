/* mm_host.h -- the host-side helpers every unit of the library shares: the early-return macro, the device guard and the
 * device-index check.  Host code only.  Everything has internal linkage (an unnamed namespace per unit), so nothing here
 * joins the library's exported symbols. */
#ifndef MM_HOST_H
#define MM_HOST_H

#include "../../include/mmcmc.h"

#include <hip/hip_runtime.h>

/* return a failed HIP call's error from the enclosing function (statuses > 0 are hipError_t values, mmcmc.h) */
#define MM_HIP(expr)                                                                                              \
    do {                                                                                                          \
        hipError_t _e = (expr);                                                                                   \
        if (_e != hipSuccess)                                                                                     \
            return (int)_e;                                                                                       \
    } while (0)

namespace {

/* makes `dev` the calling thread's device and restores the previous one on scope exit; restores nothing when the previous
 * device could not be read.  `ok`: the device was set.  Without an argument it only saves and restores -- for a function
 * that walks several devices with plain hipSetDevice calls and must leave the caller's device as it found it. */
struct DevGuard {
    int prev = -1;
    bool ok = true;
    DevGuard()
    {
        if (hipGetDevice(&prev) != hipSuccess)
            prev = -1;
    }
    explicit DevGuard(int dev) : DevGuard() { ok = hipSetDevice(dev) == hipSuccess; }
    DevGuard(const DevGuard &) = delete;
    DevGuard &operator=(const DevGuard &) = delete;
    ~DevGuard()
    {
        if (prev >= 0)
            (void)hipSetDevice(prev);
    }
};

/* MMCMC_ERR_NO_DEVICE without a usable HIP device, MMCMC_ERR_INVALID_ARG for an index outside [0, device count) */
[[maybe_unused]] int mm_check_device(int device)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return MMCMC_ERR_NO_DEVICE;
    if (device < 0 || device >= n)
        return MMCMC_ERR_INVALID_ARG;
    return MMCMC_OK;
}

} // namespace

/* mm_nuts_api.hip, for mm_progress.hip: which rows of the last run's per-draw records (mmcmc_nuts_draw_stats) belong to the sample
 * the caller holds -- mmcmc_nuts_run_progress records every state and returns the last n_collect.  Not exported. */
struct mmcmc_nuts;
__attribute__((visibility("hidden"))) int mm_nuts_draw_stats_window(mmcmc_nuts *h, size_t first_row, size_t n_rows);

#endif /* MM_HOST_H */
