/* mm_path.h -- which kernel an MH / HMC handle runs: the one rule behind sampler_create's default, the two
 * mmcmc_*_set_kernel_variant entry points and launch_range (mm_api.hip).  Pure host functions of the facts gathered once at
 * creation; no HIP include, so tests/cpp/path_rule.cpp walks the whole table with a plain C++17 compiler.  Internal linkage:
 * nothing here joins the library's exported symbols. */
#ifndef MM_PATH_H
#define MM_PATH_H

#include "../../include/mmcmc.h"

#ifndef MM_SAMPLER_MH /* mm_kernels.h's values */
#define MM_SAMPLER_MH 0
#define MM_SAMPLER_HMC 1
#endif

/* the public variant numbers of mmcmc_{mh,hmc}_set_kernel_variant / mmcmc_hmc_kernel_variant (4 was never assigned) */
enum {
    MM_VAR_PLAIN = 0,   /* one chain per lane, one iteration's noise at a time */
    MM_VAR_PIPE1 = 1,   /* alias kept: PIPE = 1 measured equal to 2 and is no longer instantiated; stored as 1, runs as 2 */
    MM_VAR_PAIRED = 2,  /* noise of two iterations packed + pipelined (PIPE = 2) */
    MM_VAR_LG = 3,      /* lane groups + MFMA (mm_hmc_lg.h): HMC, GaussianND of dim 16 or 32 */
    MM_VAR_SPLIT = 5,   /* noise waves + transition waves (mm_split_kernels.h), up to dim 8 */
    MM_VAR_GENERIC = 6, /* run-time dimension (mm_generic.h) */
    MM_VAR_UNIT = 7,    /* run-time compiled unit (mm_rtc.hip): a caller's target, or a built-in's own functor */
    MM_VAR_WIDE = 8,    /* one chain per workgroup (mm_wide.hip): HMC, a huge dimension */
    MM_VAR_MAX = 8
};

enum mm_unit_state {
    MM_UNIT_NONE = 0,
    MM_UNIT_CALLER,  /* a kind handed out by mmcmc_target_register_source / mmcmc_proposal_register_source */
    MM_UNIT_BUILTIN  /* a built-in target without a fixed-dimension kernel, dim <= 32, compiled on first use and verified */
};

/* what sampler_create learns about a handle, once */
struct mm_path_caps {
    int sampler = MM_SAMPLER_MH;
    int dtype = MMCMC_F32;
    int dim = 0;
    bool fixed = false;       /* a fixed-dimension entry (mm_kernel_entry) exists: run_mh .. run_hmc_pp10 are never null */
    bool split = false;       /* ... and it has run_mh_split / run_hmc_split / run_hmc_split10 */
    bool pp_sched = false;    /* ... and run_hmc_pp_sched */
    bool split_sched = false; /* ... and run_hmc_split_sched */
    mm_unit_state unit = MM_UNIT_NONE;
    bool generic_ok = false;  /* the target kind has a run-time-dimension form */
    bool generic_lds = false; /* ... whose per-chain store fits LDS (without a fixed entry an HBM store stands in) */
    bool wide_ok = false;
    bool lg_ok = false;
    bool few_chains = false;  /* dim >= 128 && n_chains < 1024: where the wide kernel is the default */
    bool metric = false;      /* HMC: a diagonal metric is set (mmcmc_hmc_set_metric): the handle runs its metric unit, variant 7,
                                 whatever it ran before; cleared again with the metric */
    bool dense = false;       /* ... and it is a dense one (mmcmc_hmc_set_metric_dense): only with `metric`; the same rule, the kernel
                                 of the handle's dense-metric unit */
};

/* one enumerator per launcher launch_range can call */
enum mm_launch {
    MM_LAUNCH_PLAIN,       /* run_mh / run_hmc */
    MM_LAUNCH_PP,          /* run_mh_pp / run_hmc_pp */
    MM_LAUNCH_PP10,        /* run_hmc_pp10 */
    MM_LAUNCH_SPLIT,       /* run_mh_split / run_hmc_split */
    MM_LAUNCH_SPLIT10,     /* run_hmc_split10 */
    MM_LAUNCH_PP_SCHED,    /* run_hmc_pp_sched */
    MM_LAUNCH_SPLIT_SCHED, /* run_hmc_split_sched */
    MM_LAUNCH_UNIT,        /* mm_rtc_launch_run_split, else mm_rtc_launch_run: decided by what the runtime answers */
    MM_LAUNCH_GENERIC,     /* mm_launch_run_generic_* */
    MM_LAUNCH_WIDE,        /* mm_launch_hmc_wide_* */
    MM_LAUNCH_LG,          /* mm_launch_hmc_lg / mm_launch_hmc_lg32 */
    MM_LAUNCH_SEGMENTED,   /* a scheduled run without a scheduled kernel: one unscheduled launch per run of equal (eps, L) */
    MM_LAUNCH_METRIC,      /* the HMC kernel of the handle's metric unit (mm_rtc_metric_unit): mm_rtc_launch_run with mm_run_metric_args */
    MM_LAUNCH_DENSE_METRIC /* the one of its dense-metric unit (mm_rtc_dense_metric_unit): mm_rtc_launch_run with mm_run_dense_args */
};

/* no fixed-dimension kernel and not a caller's unit: the run-time-dimension kernel is what the handle falls back on */
static inline bool mm_path_generic(const mm_path_caps &c) { return !c.fixed && c.unit != MM_UNIT_CALLER; }

/* what sampler_create guarantees about the caps of a handle it returns; the three functions below are defined on such caps */
static inline bool mm_path_caps_consistent(const mm_path_caps &c)
{
    const bool hmc = c.sampler == MM_SAMPLER_HMC;
    if ((c.split || c.pp_sched || c.split_sched) && !c.fixed)
        return false; /* launchers of an entry that does not exist */
    if (c.split_sched && !c.split)
        return false;
    if (c.unit != MM_UNIT_NONE && c.fixed)
        return false; /* a user kind has no table entry; a built-in gets a unit only for want of one */
    if (c.unit == MM_UNIT_BUILTIN && c.dim > 32)
        return false;
    if (mm_path_generic(c) && !c.generic_ok)
        return false; /* creation fails with MMCMC_ERR_UNSUPPORTED: there is no kernel at all */
    if (c.generic_lds && !c.generic_ok)
        return false;
    if (c.wide_ok && (!hmc || c.unit != MM_UNIT_NONE || c.dim < 4))
        return false;
    if (c.lg_ok && (!hmc || !c.fixed || (c.dim != 16 && c.dim != 32)))
        return false; /* GaussianND has fixed entries at 16 and 32 */
    if (c.few_chains && c.dim < 128)
        return false;
    if (c.metric && (!hmc || c.dim > 32))
        return false; /* mm_metric_status refused it */
    if (c.dense && !c.metric)
        return false; /* a dense metric is a metric */
    return true;
}

/* may a handle take a metric?  HMC up to dim 32, whatever mapping it runs now (lane groups and the wide kernel have no
 * metric form: the handle moves to its metric unit); the run-time compiler is asked for afterwards */
static inline int mm_metric_status(const mm_path_caps &c)
{
    return c.sampler == MM_SAMPLER_HMC && c.dim >= 1 && c.dim <= 32 ? MMCMC_OK : MMCMC_ERR_UNSUPPORTED;
}

static inline int mm_default_variant(const mm_path_caps &c)
{
    if (c.unit != MM_UNIT_NONE)
        return MM_VAR_UNIT;
    if (!c.fixed) /* few chains of a huge dimension: the coordinates of a chain across a workgroup */
        return c.wide_ok && c.few_chains ? MM_VAR_WIDE : MM_VAR_GENERIC;
    if (c.lg_ok)
        return MM_VAR_LG;
    /* f32 up to dim 8: four waves per SIMD (config 3: 0.192 ms against 0.268 ms for variant 2) */
    if (c.dtype == MMCMC_F32 && c.split)
        return MM_VAR_SPLIT;
    /* above dim 16 the paired form holds four noise vectors next to the state and spills: the plain form is twice as fast
     * there (RosenbrockND(32) f32: 1.0 ms vs 2.2 ms for run(100, 20) of 65 536 chains) */
    return c.dim > 16 ? MM_VAR_PLAIN : MM_VAR_PAIRED;
}

/* MMCMC_OK: the handle may be set to `variant`; MMCMC_ERR_INVALID_ARG: no such variant for this sampler;
 * MMCMC_ERR_UNSUPPORTED: not on this handle */
static inline int mm_variant_status(const mm_path_caps &c, int variant)
{
    if (variant < 0 || variant > MM_VAR_MAX || variant == 4)
        return MMCMC_ERR_INVALID_ARG;
    if (c.sampler == MM_SAMPLER_MH && (variant == MM_VAR_LG || variant == MM_VAR_WIDE))
        return MMCMC_ERR_INVALID_ARG;
    if (c.metric) /* only the metric unit has kernels that read a metric */
        return variant == MM_VAR_UNIT ? MMCMC_OK : MMCMC_ERR_UNSUPPORTED;
    if (c.unit == MM_UNIT_BUILTIN) /* its run-time compiled register kernels, or the run-time-dimension kernel they are checked against */
        return variant == MM_VAR_GENERIC || variant == MM_VAR_UNIT ? MMCMC_OK : MMCMC_ERR_UNSUPPORTED;
    if (c.unit == MM_UNIT_CALLER)
        return variant == MM_VAR_UNIT ? MMCMC_OK : MMCMC_ERR_UNSUPPORTED;
    if (variant == MM_VAR_WIDE) /* asked before the next rule: a handle without a fixed kernel may still go wide */
        return c.wide_ok ? MMCMC_OK : MMCMC_ERR_UNSUPPORTED;
    if (!c.fixed)
        return variant == MM_VAR_GENERIC ? MMCMC_OK : MMCMC_ERR_UNSUPPORTED;
    switch (variant) {
    case MM_VAR_GENERIC: /* on request next to a fixed kernel: only where the chain vectors fit LDS */
        return c.generic_ok && c.generic_lds ? MMCMC_OK : MMCMC_ERR_UNSUPPORTED;
    case MM_VAR_LG:
        return c.lg_ok ? MMCMC_OK : MMCMC_ERR_UNSUPPORTED;
    case MM_VAR_SPLIT:
        return c.split ? MMCMC_OK : MMCMC_ERR_UNSUPPORTED;
    case MM_VAR_UNIT: /* looks like a bug: accepted and reported as 7 on a handle that has no unit; runs PIPE = 2 (mm_launch_path) */
    default:
        return MMCMC_OK;
    }
}

/* the launcher of a run on a handle set to `variant` (one mm_variant_status allows); scheduled: (eps, L) per transition */
static inline mm_launch mm_launch_path(const mm_path_caps &c, int variant, int n_leapfrog, bool scheduled)
{
    const bool hmc = c.sampler == MM_SAMPLER_HMC, l10 = hmc && n_leapfrog == 10;
    if (c.metric) /* one kernel, run-time L; a schedule goes through the segmented fallback */
        return scheduled ? MM_LAUNCH_SEGMENTED : c.dense ? MM_LAUNCH_DENSE_METRIC : MM_LAUNCH_METRIC;
    if (scheduled) {
        /* kernels that read the schedule on the device: the split kernel and PIPE = 2 of the fixed-dimension targets */
        if (hmc && c.fixed && variant == MM_VAR_SPLIT && c.split_sched)
            return MM_LAUNCH_SPLIT_SCHED;
        if (hmc && c.fixed && (variant == MM_VAR_PIPE1 || variant == MM_VAR_PAIRED) && c.pp_sched)
            return MM_LAUNCH_PP_SCHED;
        return MM_LAUNCH_SEGMENTED;
    }
    switch (variant) {
    case MM_VAR_UNIT:
        if (c.unit != MM_UNIT_NONE)
            return MM_LAUNCH_UNIT;
        break; /* looks like a bug: 7 without a unit runs PIPE = 2 */
    case MM_VAR_WIDE:
        if (c.wide_ok)
            return MM_LAUNCH_WIDE;
        break;
    case MM_VAR_GENERIC:
        return MM_LAUNCH_GENERIC;
    case MM_VAR_LG:
        if (c.lg_ok)
            return MM_LAUNCH_LG;
        break;
    case MM_VAR_SPLIT:
        return l10 ? MM_LAUNCH_SPLIT10 : MM_LAUNCH_SPLIT;
    case MM_VAR_PLAIN:
        return MM_LAUNCH_PLAIN;
    default: /* 2, and 1 which selects it */
        break;
    }
    return l10 ? MM_LAUNCH_PP10 : MM_LAUNCH_PP;
}

#endif /* MM_PATH_H */
