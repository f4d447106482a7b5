/* mm_nuts_plan.h -- the host rules a NUTS handle (mm_nuts_api.hip) runs on: how run()'s arguments become transitions and
 * output rows, which kernels a handle launches, and how a lane-group run is scheduled.  Pure host functions; no HIP include, so
 * tests/cpp/nuts_plan.cpp walks them with a plain C++17 compiler.  Internal linkage: nothing here joins the library's
 * exported symbols. */
#ifndef MM_NUTS_PLAN_H
#define MM_NUTS_PLAN_H

#include "../../include/mmcmc.h"

#define MM_NUTS_PLAN_JMAX 12    /* mm_nuts.h's MM_NUTS_JMAX */
#define MM_NUTS_PLAN_ID_BITS 20 /* mm_nuts_lg.h's MM_LGQ_ID_BITS */
#ifndef MM_NUTS_JMAX
#define MM_NUTS_JMAX MM_NUTS_PLAN_JMAX
#endif
#ifndef MM_LGQ_ID_BITS
#define MM_LGQ_ID_BITS MM_NUTS_PLAN_ID_BITS
#endif

/* ---------------------------------------------------------------- step plan */

/* run(n_collect, n_discard) as the kernels take it: n_pre transitions without output, then n_rec recorded ones, the current
 * position first as a row of its own if write_initial; n_rows rows per chain in all */
struct mm_nuts_steps {
    int status;
    size_t n_rows;
    unsigned int write_initial, n_pre, n_rec;
};
/* progress 0: NUTS::run (nuts.rs:457-471): N - 1 transitions, row 0 is the initial point; 1: run_progress (nuts.rs:491-522):
 * all N transitions, the last n_collect recorded; 2: run_progress' stepping with EVERY state recorded, burn-in included (what
 * the per-chain trackers of nuts.rs:486-506 are fed).  m: the transitions taken so far.  Row indices and the step counter are
 * 32-bit in the kernels: n_rows * dim < 2^30 and m + n_collect + n_discard < 2^32 */
static inline mm_nuts_steps mm_nuts_step_plan(size_t n_collect, size_t n_discard, int progress, int dim, uint32_t m)
{
    mm_nuts_steps s = {MMCMC_OK, 0, 0u, 0u, 0u};
    if (progress < 0 || progress > 2) {
        s.status = MMCMC_ERR_INVALID_ARG;
        return s;
    }
    s.n_rows = progress == 2 ? n_collect + n_discard : n_collect;
    if ((uint64_t)s.n_rows * (uint64_t)dim >= (1ull << 30) || (uint64_t)m + n_collect + n_discard >= (1ull << 32)) {
        s.status = MMCMC_ERR_SHAPE;
        return s;
    }
    const size_t total = n_collect + n_discard;
    if (progress == 2) {
        s.n_rec = (unsigned int)total;
    } else if (progress) {
        s.n_pre = (unsigned int)n_discard;
        s.n_rec = (unsigned int)n_collect;
    } else if (total == 0) {
        /* nothing to do */
    } else if (n_discard == 0) {
        s.write_initial = 1u;
        s.n_rec = (unsigned int)(n_collect - 1);
    } else {
        s.n_pre = (unsigned int)(n_discard - 1);
        s.n_rec = (unsigned int)n_collect;
    }
    return s;
}

/* ---------------------------------------------------------------- path rule */

/* the public variant numbers of mmcmc_nuts_set_kernel_variant / mmcmc_nuts_kernel_variant */
enum {
    MM_NVAR_STEP = 0,      /* one chain per lane, the lanes of a wave in step */
    MM_NVAR_LG = 1,        /* lane groups / MFMA (mm_nuts_lg.h), one launch */
    MM_NVAR_LG_LEVELS = 2, /* ... with tree-depth compaction, one launch per level */
    MM_NVAR_LG_QUEUE = 3,  /* ... with compaction by a persistent scheduler */
    MM_NVAR_ASYNC = 4,     /* one chain per lane, asynchronous lanes */
    MM_NVAR_PAIR = 5,      /* asynchronous lanes, leaves in pairs */
    MM_NVAR_GENERIC = 6,   /* run-time dimension (mm_nuts_generic.h) */
    MM_NVAR_UNIT = 7,      /* run-time compiled unit (mm_rtc.hip) */
    MM_NVAR_MAX = 7
};
/* mm_metric_host.h's MM_METRIC_* */
enum { MM_NMETRIC_NONE = 0, MM_NMETRIC_DIAG = 1, MM_NMETRIC_DENSE = 2 };

/* what setup() learns about a handle, once */
struct mm_nuts_caps {
    bool inst = false;       /* a compiled (kind, dim) instance exists (mm_nuts_entry): init and run are never null */
    bool inst_async = false; /* ... and it has run_async */
    bool inst_pair = false;  /* ... and run_pair */
    bool lg = false;         /* a lane-group entry (mm_nuts_lg_entry): <double, double>, GaussianND, dim 16 or 32 */
    bool generic_ok = false; /* the target kind has a run-time-dimension form */
    bool unit = false;       /* a run-time compiled unit of the target: a caller's kind, or a built-in's for want of an instance */
};
/* what setup() guarantees about the caps of a handle it returns; the three functions below are defined on such caps */
static inline bool mm_nuts_caps_consistent(const mm_nuts_caps &c)
{
    if ((c.inst_async || c.inst_pair) && !c.inst)
        return false; /* launchers of an entry that does not exist */
    if (c.unit && c.inst)
        return false; /* a user kind has no table entry; a built-in gets a unit only for want of one */
    return c.inst || c.unit || c.generic_ok; /* else creation fails with MMCMC_ERR_UNSUPPORTED: there is no kernel at all */
}

/* one enumerator per launcher run() can reach */
enum mm_nuts_launch {
    MM_NLAUNCH_NONE,        /* no variant mm_nuts_variant_status allows leads here */
    MM_NLAUNCH_INST_STEP,   /* the instance's run */
    MM_NLAUNCH_INST_ASYNC,  /* its run_async */
    MM_NLAUNCH_INST_PAIR,   /* its run_pair */
    MM_NLAUNCH_LG,          /* the lane-group entry (run_lg decides how: mm_nuts_lg_mode) */
    MM_NLAUNCH_GENERIC,     /* mm_launch_nuts_generic_* */
    MM_NLAUNCH_TARGET_UNIT, /* the kernels of the target's run-time compiled unit */
    MM_NLAUNCH_METRIC_UNIT, /* the handle's diagonal-metric unit (mm_rtc_metric_unit) */
    MM_NLAUNCH_DENSE_UNIT,  /* its dense-metric unit */
    MM_NLAUNCH_STATS_UNIT,  /* its stats unit (mm_rtc_stats_unit) without a metric, + MM_NMETRIC_DIAG / _DENSE: the two below */
    MM_NLAUNCH_STATS_UNIT_DIAG,
    MM_NLAUNCH_STATS_UNIT_DENSE
};

/* lane groups where they exist; else asynchronous lanes with the leaves in pairs, the default of the one-chain-per-lane
 * kernels; without an instance the target's unit, else the run-time-dimension kernel */
static inline int mm_nuts_default_variant(const mm_nuts_caps &c)
{
    if (c.lg)
        return MM_NVAR_LG_QUEUE;
    if (c.inst)
        return c.inst_pair ? MM_NVAR_PAIR : c.inst_async ? MM_NVAR_ASYNC : MM_NVAR_STEP;
    return c.unit ? MM_NVAR_UNIT : MM_NVAR_GENERIC;
}

/* MMCMC_OK: the handle may be set to `variant`; MMCMC_ERR_INVALID_ARG: no such variant; MMCMC_ERR_UNSUPPORTED: not on this
 * handle.  Only the metric units have kernels that read a metric and only the stats units kernels that record: such a handle
 * is on variant 7 until the metric is cleared and recording is off */
static inline int mm_nuts_variant_status(const mm_nuts_caps &c, int metric, bool recording, int variant)
{
    if (variant < 0 || variant > MM_NVAR_MAX)
        return MMCMC_ERR_INVALID_ARG;
    bool ok = false;
    if (metric != MM_NMETRIC_NONE || recording)
        ok = variant == MM_NVAR_UNIT;
    else
        switch (variant) {
        case MM_NVAR_STEP: ok = c.inst; break;
        case MM_NVAR_LG:
        case MM_NVAR_LG_LEVELS:
        case MM_NVAR_LG_QUEUE: ok = c.lg; break;
        case MM_NVAR_ASYNC: ok = c.inst && c.inst_async; break;
        case MM_NVAR_PAIR: ok = c.inst && c.inst_pair; break;
        case MM_NVAR_GENERIC: ok = c.generic_ok; break;
        default: ok = c.unit; break;
        }
    return ok ? MMCMC_OK : MMCMC_ERR_UNSUPPORTED;
}

/* the launcher of a run on a handle set to `variant` (one mm_nuts_variant_status allows) */
static inline mm_nuts_launch mm_nuts_launch_path(const mm_nuts_caps &c, int metric, bool recording, int variant)
{
    if (mm_nuts_variant_status(c, metric, recording, variant) != MMCMC_OK)
        return MM_NLAUNCH_NONE;
    if (recording)
        return (mm_nuts_launch)(MM_NLAUNCH_STATS_UNIT + metric);
    if (metric != MM_NMETRIC_NONE)
        return metric == MM_NMETRIC_DENSE ? MM_NLAUNCH_DENSE_UNIT : MM_NLAUNCH_METRIC_UNIT;
    switch (variant) {
    case MM_NVAR_STEP: return MM_NLAUNCH_INST_STEP;
    case MM_NVAR_ASYNC: return MM_NLAUNCH_INST_ASYNC;
    case MM_NVAR_PAIR: return MM_NLAUNCH_INST_PAIR;
    case MM_NVAR_GENERIC: return MM_NLAUNCH_GENERIC;
    case MM_NVAR_UNIT: return MM_NLAUNCH_TARGET_UNIT;
    default: return MM_NLAUNCH_LG;
    }
}

/* ---------------------------------------------------------------- lane-group schedule */

/* a measurement knob (mm_tuning.h) as the caller read it; absent in an ordinary build */
struct mm_knob {
    bool set = false;
    int value = 0;
};

enum mm_nuts_lg_sched {
    MM_NLG_SINGLE,    /* one launch, every wave keeps its chains */
    MM_NLG_QUEUE,     /* the persistent scheduler */
    MM_NLG_PER_LEVEL  /* one launch per level and transition, in chain groups */
};
/* total = the run's transitions.  Few chains cannot fill the queues of a scheduler; its queue entries hold a chain index in
 * MM_LGQ_ID_BITS bits, so variant 3 on more chains than that runs as variant 2 */
static inline mm_nuts_lg_sched mm_nuts_lg_mode(int variant, unsigned int total, size_t n_chains, size_t c_pad)
{
    if (variant == MM_NVAR_LG || total == 0 || (variant == MM_NVAR_LG_QUEUE && n_chains < 2048))
        return MM_NLG_SINGLE;
    if (variant == MM_NVAR_LG_QUEUE && c_pad < ((size_t)1 << MM_LGQ_ID_BITS))
        return MM_NLG_QUEUE;
    return MM_NLG_PER_LEVEL;
}

/* idle polls before a scheduler wave settles for less than a full unit.  Round 2 (65 536 chains): 4 -> 516.5 ms, 16 -> 518.5,
 * 64 -> 520.9, 256 -> 530.3; round 6, with the leaf loop 25 % faster: 0 / 1 / 2 / 4 / 8 -> 347.9 / 348.0 / 348.5 / 349.3 /
 * 349.7 ms at 15.75-15.77 chains per unit (profiles/r6zh_lgq_patience.log): waiting buys no fuller units */
static const unsigned int mm_nuts_lgq_patience = 1u;
/* a wave stays with the chains it kept only when the queue of their level makes a FULL unit of them; else they are queued and
 * the wave takes the deepest full unit there is (config 5 with the edges in registers: 10 -> 408.6 ms, 12 -> 390.1, 14 ->
 * 381.2, 16 -> 377.5: 15.27 -> 15.78 chains per unit; profiles/r5zzz_lgq_min_unit.log) */
static const unsigned int mm_nuts_lgq_min_unit = 16u;
/* transitions a fresh handle runs at the default level to have a depth histogram (mm_nuts_pilot_split) */
static const unsigned int mm_nuts_lgq_pilot = 16u;

/* the persistent scheduler's grid: nw waves, built for occ waves per SIMD (mm_lg_cfg).  One resident wave per SIMD, fewer if
 * there are fewer groups of 16 chains; two per SIMD only where the handle asks for it (lgq_occ, or the MMCMC_LGQ_OCC knob)
 * and both can be filled.  The MMCMC_LGQ_WAVES knob can only lower nw */
struct mm_nuts_lgq_shape {
    unsigned int nw;
    int occ;
};
static inline mm_nuts_lgq_shape mm_nuts_lgq_grid(unsigned int groups16, unsigned int resident_waves, int lgq_occ, mm_knob occ_knob,
                                                 mm_knob waves_knob)
{
    int occ = occ_knob.set ? (occ_knob.value == 2 ? 2 : 1) : lgq_occ;
    if (groups16 < 2u * resident_waves)
        occ = 1;
    const unsigned int resident = resident_waves * (unsigned int)occ;
    unsigned int nw = groups16 < resident ? groups16 : resident;
    if (waves_knob.set) {
        const unsigned int w = (unsigned int)waves_knob.value;
        if (w >= 1 && w < nw)
            nw = w;
    }
    return {nw, occ};
}

/* The first compaction level pays when it sits just below the depth most trees reach (config 5, trees 7 - 8 deep: level 5
 * 660 ms, 7 648 ms, 8 782 ms at 65 536 chains; 234 -> 203 ms at 16 384).  Unless the caller fixed it, it is the mode of the
 * handle's depth histogram [MM_NUTS_JMAX + 1] minus one, within [3, max_depth], once the histogram holds 8 transitions per
 * chain; -1 before that */
static inline int mm_nuts_level_from_hist(const unsigned int *hist, size_t n_chains, int max_depth)
{
    unsigned long long sum = 0;
    int mode = 0;
    for (int i = 0; i <= MM_NUTS_JMAX; ++i) {
        sum += hist[i];
        if (hist[i] > hist[mode])
            mode = i;
    }
    if (sum < 8ull * n_chains)
        return -1;
    const int l = mode - 1 < 3 ? 3 : mode - 1;
    return l < max_depth ? l : max_depth;
}

/* a stretch of a run as one launch takes it (the fields of the same names in mm_nuts_args) */
struct mm_nuts_segment {
    unsigned int m0, n_pre, n_rec, write_initial, out_t0;
};
/* A fresh handle has no histogram: a run of at least 4 * pilot transitions takes its first `pilot` ones as a launch of their
 * own, after which the level is read.  Splitting a run never changes a result (the stream is keyed by chain and step): the
 * second launch goes on at step m0 + pilot, behind the rows the first one wrote */
struct mm_nuts_pilot_plan {
    int n; /* 1: seg[0] is the run; 2: the pilot, then the rest */
    mm_nuts_segment seg[2];
};
static inline mm_nuts_pilot_plan mm_nuts_pilot_split(const mm_nuts_segment &a, bool level_known, unsigned int pilot)
{
    mm_nuts_pilot_plan p = {1, {a, a}};
    if (level_known || a.n_pre + a.n_rec < 4 * pilot)
        return p;
    mm_nuts_segment &s1 = p.seg[0], &s2 = p.seg[1];
    p.n = 2;
    s1.n_pre = a.n_pre < pilot ? a.n_pre : pilot;
    s1.n_rec = pilot - s1.n_pre;
    s2.m0 = a.m0 + pilot;
    s2.n_pre = a.n_pre - s1.n_pre;
    s2.n_rec = a.n_rec - s1.n_rec;
    s2.write_initial = 0u;
    s2.out_t0 = a.out_t0 + (a.write_initial ? 1u : 0u) + s1.n_rec;
    return p;
}

/* Tree-depth compaction by launches: 1 + (max_depth - j0) launches per transition.  The late launches of a transition hold few
 * chains (a few per cent reach the deepest level), so the chains are split into groups, each with its own launch sequence on
 * its own stream: one group's narrow launches run beside another's wide ones.  Groups are contiguous blocks of whole 16-chain
 * waves: `requested` of them (0: one per 16 384 chains), at most MM_NUTS_LG_MAX_GROUPS and at most one per wave */
#define MM_NUTS_LG_MAX_GROUPS 16
static inline int mm_nuts_lg_n_groups(int requested, size_t n_chains, size_t c_pad)
{
    int n = requested > 0 ? requested : (int)(n_chains / 16384);
    n = n < 1 ? 1 : (n > MM_NUTS_LG_MAX_GROUPS ? MM_NUTS_LG_MAX_GROUPS : n);
    const size_t waves = c_pad / 16;
    return (size_t)n > waves ? (int)waves : n;
}
/* group gi of n_groups: the waves [w0, w1), the chains [offset, offset + n_chains), c_pad of them with the padding */
struct mm_nuts_lg_group {
    size_t w0, w1, offset, n_chains, c_pad;
};
static inline mm_nuts_lg_group mm_nuts_lg_group_of(int gi, int n_groups, size_t n_chains, size_t c_pad)
{
    const size_t waves = c_pad / 16;
    const size_t w0 = waves * (size_t)gi / (size_t)n_groups, w1 = waves * ((size_t)gi + 1) / (size_t)n_groups;
    return {w0, w1, w0 * 16, (w1 * 16 < n_chains ? w1 * 16 : n_chains) - w0 * 16, (w1 - w0) * 16};
}
/* transition t of the run `a`, as the per-level kernels take it: m the 1-based step, row its output row or 0xffffffff */
struct mm_nuts_lg_step {
    unsigned int m, write_initial, row;
};
static inline mm_nuts_lg_step mm_nuts_lg_step_of(const mm_nuts_segment &a, unsigned int t)
{
    return {a.m0 + t + 1, t == 0 ? a.write_initial : 0u,
            t >= a.n_pre ? a.out_t0 + (a.write_initial ? 1u : 0u) + (t - a.n_pre) : 0xffffffffu};
}

#endif /* MM_NUTS_PLAN_H */
