/*
 * mm_nuts_api.hip -- C ABI of the NUTS sampler (include/mmcmc.h: mmcmc_nuts_*).  Host logic only.
 * Mirrors NUTS::{new, set_seed, run, run_progress} (nuts.rs:123-170, 194-353) over NUTSChain (nuts.rs:410-691).
 */
#include "../../include/mmcmc.h"
#include "mm_host.h"
#include "mm_metric_host.h"
#include "mm_hostcopy.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <mutex>
#include <map>
#include <vector>

#include <type_traits>

#include "mm_nuts_kernels.h"
#include "mm_nuts_lg.h"
#include "mm_nuts_generic.h"
#include "mm_tuning.h"
#include "mm_rtc.h"
#include "mm_params.h"
#include "mm_nuts_plan.h"

static_assert(MM_NUTS_JMAX == MM_NUTS_PLAN_JMAX && MM_LGQ_ID_BITS == MM_NUTS_PLAN_ID_BITS, "mm_nuts_plan.h's copies of the kernel headers' constants");
static_assert(MM_NMETRIC_NONE == MM_METRIC_NONE && MM_NMETRIC_DIAG == MM_METRIC_DIAG && MM_NMETRIC_DENSE == MM_METRIC_DENSE &&
                  MM_NVAR_UNIT == mm_metric_variant,
              "mm_nuts_plan.h's metric kinds are mm_metric_host.h's; a handle with a metric is on variant 7");
/* the layout rules as functions of run-time sizes (mm_kernels.h, mm_nuts_kernels.h) against the templates' values */
static_assert(mm_nuts_stack_bytes(4, 8, 3) == mm_nuts_stack_layout<float, double, 3>::bytes && mm_nuts_stack_layout<float, double, 3>::bytes == 43008 &&
                  mm_nuts_stack_bytes(4, 4, 9) == mm_nuts_stack_layout<float, float, 9>::bytes &&
                  mm_nuts_stack_bytes(8, 8, 32) == mm_nuts_stack_layout<double, double, 32>::bytes &&
                  mm_tile_lds_bytes_per_wave(4, 9, mm_tile_default_t(4, 9)) == mm_tile<float, 9>::lds_bytes_per_wave &&
                  mm_tile_lds_bytes_per_wave(8, 32, mm_tile_default_t(8, 32)) == mm_tile<double, 32>::lds_bytes_per_wave,
              "the run-time layout rules are the templates'");

namespace {

/* a measurement knob (mm_tuning.h): absent in an ordinary build */
inline mm_knob knob(const char *name)
{
    mm_knob k;
    if (const char *ev = mm_tuning_env(name)) {
        k.set = true;
        k.value = atoi(ev);
    }
    return k;
}

/* the fields every NUTS argument struct has under the same name, from the run's mm_nuts_args */
template <class Q, class A> Q shared_nuts_args(const A &a)
{
    Q q;
    q.state = a.state;
    q.adapt = a.adapt;
    q.out = a.out;
    q.n_leapfrog = a.n_leapfrog;
    q.depth_hist = a.depth_hist;
    q.n_chains = a.n_chains;
    q.seed = a.seed;
    q.chain_offset = a.chain_offset;
    q.n_total = a.n_total;
    q.m0 = a.m0;
    q.n_pre = a.n_pre;
    q.n_rec = a.n_rec;
    q.write_initial = a.write_initial;
    q.out_t0 = a.out_t0;
    q.n_discard = a.n_discard;
    q.max_depth = a.max_depth;
    q.target_accept_p = a.target_accept_p;
    return q;
}

/* 0: normal; 1: inside the self-test of a run-time compiled unit; 2: create without run-time compiled built-in units */
thread_local int g_rtc_create_mode = 0;

struct NutsBase {
    virtual ~NutsBase() {}
    virtual int run(size_t n_collect, size_t n_discard, void *out, int out_is_device, int progress, void *stream) = 0;
    virtual int state(void *out) = 0;
    virtual int adapt_state(double *out) = 0;
    virtual int set_state(const void *x, int is_device, void *stream) = 0;
    virtual int set_adapt_state(const double *in) = 0;
    virtual int leapfrog_counts(uint64_t *out) = 0;
    virtual int depth_histogram(uint32_t *out) = 0;
    virtual int set_metric(bool dense, const double *values) = 0;
    virtual int set_draw_stats(bool on) = 0;
    virtual int draw_stats(mmcmc_nuts_draw *out, int out_is_device, size_t *n_rows) = 0;
    virtual int draw_stats_window(size_t first, size_t rows) = 0;
    mm_nuts_caps caps; /* what setup() found for the handle: the facts the kernel-path rule (mm_nuts_plan.h) works on */
    int set_variant(int v)
    {
        const int st = mm_nuts_variant_status(caps, met.kind, recording, v);
        if (st == MMCMC_OK) /* with a metric or while recording this is 7, which the handle is on */
            variant = v;
        return st;
    }
    mm_metric_record met; /* the metric that is set (mmcmc_nuts_set_metric, _set_metric_dense; mm_metric_host.h) */
    /* per-draw statistics (mmcmc_nuts_set_draw_stats): while on the handle runs a stats unit, variant 7, like a handle with a
     * metric.  The variant to return to is kept once: by `met` while a metric is set, else here. */
    bool recording = false;
    int variant_before_recording = 0;
    int variant = 0; /* MM_NVAR_* (mm_nuts_plan.h): always one mm_nuts_variant_status allows on this handle */
    int compaction_start = 5; /* variants 2, 3: doublings below this run before the first compaction */
    bool compaction_auto = true; /* variant 3: choose it from the depths seen so far (until set_compaction is called) */
    int compaction_groups = 0; /* variant 2: chain groups with their own launch sequence (0 = choose) */
    int device = 0, mode = 0, kind = 0, dim = 0;
    const void *rtc_unit = nullptr; /* the run-time compiled unit whose kernels this handle launches (mm_rtc.hip), or NULL */
    int rtc_run_kernel = 2; /* which of the unit's run kernels: 2 asynchronous lanes, leaves in pairs (what handles launch);
                               0 the lanes in step (launched only by rtc_unit_verified, as the second opinion on a user target) */
    size_t n_chains = 0;
    uint64_t seed = 0, chain_offset = 0;
    uint32_t m = 0; /* self.m: transitions taken so far */
    int max_depth = 10;
    double target_accept_p = 0.8;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    mmcmc_timing timing{};
};

template <class TT, class ST> const mm_nuts_entry<TT, ST> *nuts_table(int *n);
template <> const mm_nuts_entry<float, double> *nuts_table<float, double>(int *n) { return mm_nuts_table_m0(n); }
template <> const mm_nuts_entry<float, float> *nuts_table<float, float>(int *n) { return mm_nuts_table_m1(n); }
template <> const mm_nuts_entry<double, double> *nuts_table<double, double>(int *n) { return mm_nuts_table_m2(n); }

inline hipError_t launch_generic(const mm_gen_nuts_args<float, double> &a, int init, hipStream_t st) { return mm_launch_nuts_generic_m0(a, init, st); }
inline hipError_t launch_generic(const mm_gen_nuts_args<float, float> &a, int init, hipStream_t st) { return mm_launch_nuts_generic_m1(a, init, st); }
inline hipError_t launch_generic(const mm_gen_nuts_args<double, double> &a, int init, hipStream_t st) { return mm_launch_nuts_generic_m2(a, init, st); }

template <class TT, class ST> struct Nuts : NutsBase {
    const mm_nuts_entry<TT, ST> *k = nullptr;
    /* run-time-dimension path (mm_nuts_generic.h, variant 6): the only one where the table has no (kind, dim) entry */
    bool generic_ok = false;
    const mm_user_target *user = nullptr; /* run-time compiled target (mm_rtc.hip, variant 7) */
    size_t user_stack_bytes = 0, user_lds = 0;
    /* with a metric: the diagonal or the dense unit whose kernels read it (mm_rtc_metric_unit), d_metric = s, then r = TT(1) / s,
     * or L, then L^-1, each packed by rows, in the tensor type (metric_image; the buffer has room for either form: 2
     * mm_tri_len(dim) elements), and the stack area of the units' kernels (a handle on a compiled instance keeps its stack in LDS
     * and has none of its own) */
    const mm_user_target *metric_unit = nullptr, *dense_unit = nullptr;
    TT *d_metric = nullptr;
    unsigned char *d_metric_scratch = nullptr;
    /* while recording: the stats unit per metric kind (mm_rtc_stats_unit; its kernels' stack is d_metric_scratch too), and the
     * records of the last run, d_rec [n_chains, rec_stride] of which rows rec_first .. rec_first + rec_rows are the rows of the
     * sample the caller got (run_progress records every row and returns the last n_collect) */
    const mm_user_target *stats_unit[3] = {nullptr, nullptr, nullptr};
    mm_nuts_draw *d_rec = nullptr;
    size_t rec_capacity = 0, rec_stride = 0, rec_first = 0, rec_rows = 0;
    bool rec_valid = false;
    TT *d_gstore = nullptr;
    int gstore_depth = 0;
    size_t g_pad = 0;
    mm_tparams<TT> P;
    TT *d_state = nullptr, *d_mat = nullptr;
    mm_nuts_adapt<ST> *d_adapt = nullptr;
    unsigned long long *d_nlf = nullptr;
    unsigned int *d_hist = nullptr;
    unsigned char *d_scratch = nullptr;
    bool stack_in_lds = true;
    const mm_nuts_lg_entry *lg = nullptr;
    double *d_lg_scratch = nullptr, *d_lg_rec = nullptr;
    unsigned int *d_lg_lists = nullptr, *d_lg_counts = nullptr;
    mm_lgq_ctrl *d_lg_ctrl = nullptr;
    unsigned int n_resident_waves = 1024;
    int lgq_occ = 1; /* waves per SIMD of the persistent scheduler (MMCMC_LGQ_OCC overrides) */
    unsigned int n_launches_run = 0; /* sampling launches of the current run() (reported by timing()) */
    int auto_level = -1;             /* first compaction level chosen from the depth histogram, once it is known */
    size_t c_pad = 0;
    static constexpr int kMaxGroups = MM_NUTS_LG_MAX_GROUPS;
    hipStream_t lg_streams[kMaxGroups] = {};
    hipEvent_t lg_fork = nullptr, lg_join[kMaxGroups] = {};

    ~Nuts() override
    {
        DevGuard g(device);
        if (stream)
            (void)hipStreamSynchronize(stream);
        (void)hipFree(d_state);
        (void)hipFree(d_mat);
        (void)hipFree(d_adapt);
        (void)hipFree(d_nlf);
        (void)hipFree(d_hist);
        (void)hipFree(d_scratch);
        (void)hipFree(d_gstore);
        (void)hipFree(d_metric);
        (void)hipFree(d_metric_scratch);
        (void)hipFree(d_rec);
        (void)hipFree(d_lg_scratch);
        (void)hipFree(d_lg_rec);
        (void)hipFree(d_lg_lists);
        (void)hipFree(d_lg_counts);
        (void)hipFree(d_lg_ctrl);
        for (int i = 0; i < kMaxGroups; ++i) {
            if (lg_streams[i])
                (void)hipStreamDestroy(lg_streams[i]);
            if (lg_join[i])
                (void)hipEventDestroy(lg_join[i]);
        }
        if (lg_fork)
            (void)hipEventDestroy(lg_fork);
        if (ev0)
            (void)hipEventDestroy(ev0);
        if (ev1)
            (void)hipEventDestroy(ev1);
        if (stream)
            (void)hipStreamDestroy(stream);
    }

    /* mm_nuts_stack_layout<TT, ST, D>::bytes and the output tile of mm_tile<TT, D>, for a run-time D: what a unit's kernels
     * take as stack area per wave and (lanes in step) as dynamic LDS */
    static void unit_sizes(size_t D, size_t *stack_bytes, size_t *tile_lds)
    {
        *stack_bytes = mm_nuts_stack_bytes(sizeof(TT), sizeof(ST), (int)D);
        *tile_lds = (mm_tile_lds_bytes_per_wave(sizeof(TT), (int)D, mm_tile_default_t(sizeof(TT), (int)D)) + 15) / 16 * 16;
    }

    static constexpr int type_mode = std::is_same<TT, double>::value ? 2 : (std::is_same<ST, double>::value ? 0 : 1);
    static constexpr ST eps_tol = sizeof(ST) == 4 ? (ST)1.1920929e-7 : (ST)2.220446049250313e-16; /* T::epsilon() */
    /* NUTSChain::new (nuts.rs:415-433): epsilon = -1 (sentinel: no search yet), epsilon_bar = 1, h_bar = 0, mu = ln 10 */
    static void fresh_adapt(std::vector<mm_nuts_adapt<ST>> &ad)
    {
        for (auto &a : ad) {
            a.epsilon = (ST)-1;
            a.epsilon_bar = (ST)1;
            a.h_bar = (ST)0;
            a.mu = (ST)std::log(10.0);
        }
    }

    /* what a run works on: the handle's own buffers and stream position (run()), or those of unit_verified's probe */
    struct Where {
        TT *state;
        mm_nuts_adapt<ST> *adapt;
        TT *out;
        unsigned long long *n_leapfrog;
        unsigned int *depth_hist;
        unsigned char *scratch;
        size_t n_chains;
        uint64_t seed, chain_offset;
        uint32_t m0;
        int max_depth;
        double target_accept_p;
        bool stack_in_lds;
    };
    /* both argument blocks of the run `s` (mm_nuts_step_plan) there */
    void fill_args(const Where &w, const mm_nuts_steps &s, size_t n_discard, mm_nuts_init_args<TT, ST> *ia, mm_nuts_args<TT, ST> *a) const
    {
        ia->P = P;
        ia->state = w.state;
        ia->adapt = w.adapt;
        ia->n_chains = w.n_chains;
        ia->seed = w.seed;
        ia->chain_offset = w.chain_offset;
        ia->eps_tol = eps_tol;
        a->P = P;
        a->state = w.state;
        a->adapt = w.adapt;
        a->out = w.out;
        a->n_leapfrog = w.n_leapfrog;
        a->depth_hist = w.depth_hist;
        a->n_chains = w.n_chains;
        a->seed = w.seed;
        a->chain_offset = w.chain_offset;
        a->n_total = s.n_rows;
        a->m0 = w.m0;
        a->n_pre = s.n_pre;
        a->n_rec = s.n_rec;
        a->write_initial = s.write_initial;
        a->out_t0 = 0;
        a->n_discard = (unsigned int)n_discard;
        a->max_depth = w.max_depth;
        a->target_accept_p = (ST)w.target_accept_p;
        a->stack_in_lds = w.stack_in_lds ? 1 : 0;
        a->async_batch = 0;
        a->scratch = w.scratch;
    }

    /* One launch of a kernel of a metric unit or of a stats unit: init_chain (which = 1), a run by the pair kernel (which = 2:
     * what handles launch) or with the lanes in step (which = 0: the second opinion of unit_verified).  The argument block is `a`
     * followed by what the unit adds, each pointer where the kernels' structs have it (mm_nuts_kernels.h: mm_nuts_*metric_args,
     * mm_nuts_*dense_args, mm_nuts_stats_args; `a` ends on a pointer boundary): the metric's image met = s, r (diagonal) or L,
     * L^-1 packed by rows (dense), then, for the run kernels of a stats unit (`stats`), the records */
    template <class A>
    hipError_t unit_launch(const mm_user_target *unit, int metric_kind, const A &a, int which, const TT *met, bool stats, mm_nuts_draw *rec,
                           size_t lds, hipStream_t st)
    {
        static_assert(sizeof(A) % sizeof(void *) == 0 && alignof(A) == alignof(void *), "the pointers follow the block without padding");
        alignas(8) unsigned char block[sizeof(A) + 3 * sizeof(void *)];
        size_t n = sizeof(A);
        std::memcpy(block, &a, n);
        auto push = [&](const void *p) {
            std::memcpy(block + n, &p, sizeof p);
            n += sizeof p;
        };
        if (metric_kind != MM_METRIC_NONE)
            push(met);
        if (metric_kind == MM_METRIC_DENSE)
            push(met + mm_tri_len((size_t)dim));
        if (stats)
            push(rec);
        return mm_rtc_launch_nuts(unit, type_mode, which, block, n, (unsigned int)((a.n_chains + 63) / 64), lds, st);
    }
    hipError_t unit_init(const mm_user_target *unit, int metric_kind, const mm_nuts_init_args<TT, ST> &ia, const TT *met, hipStream_t st)
    {
        return unit_launch(unit, metric_kind, ia, 1, met, false, nullptr, 0, st);
    }
    /* `scratch` of a = the stack area, one unit_sizes() block per wave */
    hipError_t unit_run(const mm_user_target *unit, int metric_kind, const mm_nuts_args<TT, ST> &a, int which, const TT *met, bool stats,
                        mm_nuts_draw *rec, hipStream_t st)
    {
        size_t stack = 0, tile = 0;
        unit_sizes((size_t)dim, &stack, &tile);
        return unit_launch(unit, metric_kind, a, which, met, stats, rec, which == 2 ? (size_t)MM_NUTS_RING * 64 * sizeof(double) : tile, st);
    }

    /* The metric unit is checked once per (unit, type mode) and process before a handle relies on it, like the units of
     * rtc_unit_verified, on this handle's own parameter block (a kind that carries data is checked on its data): 96 chains,
     * 5 + 5 transitions from a fixed start under a general metric, (a) twice by the pair kernel -- the same bits --, (b) by
     * the unit's lanes-in-step kernel, which must agree bit for bit, under rtc_unit_verified's condition on the compiler
     * that built the unit.  Only real verdicts are cached.
     * metric_kind MM_METRIC_DENSE: a dense-metric unit, checked the same way under a general factor with large off-diagonal
     * entries.  stats: a stats unit (mm_rtc_stats_unit) of that metric kind, MM_METRIC_NONE included: the same runs with their
     * records, and samples AND records must agree bit for bit. */
    bool unit_verified(const mm_user_target *unit, int metric_kind, bool stats)
    {
        const bool dense = metric_kind == MM_METRIC_DENSE;
        static std::mutex mu;
        static std::map<const void *, bool> verdict;
        {
            std::lock_guard<std::mutex> l(mu);
            auto it = verdict.find(unit);
            if (it != verdict.end())
                return it->second;
        }
        const size_t n = 96, D = (size_t)dim, nc = 5, nd = 5, waves = (n + 63) / 64;
        size_t stack = 0, tile = 0;
        unit_sizes(D, &stack, &tile);
        /* the probe inputs of mm_metric_host.h, as the image a setter would upload */
        const std::vector<double> start = mm_probe_start(n, D);
        const std::vector<TT> x0(start.begin(), start.end());
        std::vector<TT> met(1, TT(0)); /* no metric: a block nobody reads */
        if (metric_kind != MM_METRIC_NONE && !metric_image(dense, (dense ? mm_probe_chol(D) : mm_probe_scale(D)).data(), met))
            return false;
        std::vector<mm_nuts_adapt<ST>> ad0(n);
        fresh_adapt(ad0);
        struct Dev {
            TT *x = nullptr, *out = nullptr, *met = nullptr;
            mm_nuts_adapt<ST> *ad = nullptr;
            unsigned char *scratch = nullptr;
            mm_nuts_draw *rec = nullptr;
            ~Dev()
            {
                (void)hipFree(rec);
                (void)hipFree(x);
                (void)hipFree(out);
                (void)hipFree(met);
                (void)hipFree(ad);
                (void)hipFree(scratch);
            }
        } d;
        if (hipMalloc((void **)&d.x, n * D * sizeof(TT)) != hipSuccess || hipMalloc((void **)&d.out, n * nc * D * sizeof(TT)) != hipSuccess ||
            hipMalloc((void **)&d.met, met.size() * sizeof(TT)) != hipSuccess || hipMalloc((void **)&d.ad, n * sizeof(mm_nuts_adapt<ST>)) != hipSuccess ||
            hipMalloc((void **)&d.scratch, waves * stack) != hipSuccess || (stats && hipMalloc((void **)&d.rec, n * nc * sizeof(mm_nuts_draw)) != hipSuccess) ||
            hipMemcpy(d.met, met.data(), met.size() * sizeof(TT), hipMemcpyHostToDevice) != hipSuccess)
            return false;
        auto one = [&](int which, std::vector<TT> &got, std::vector<unsigned char> &got_rec) -> bool {
            got.assign(n * nc * D, TT(0));
            got_rec.assign(stats ? n * nc * sizeof(mm_nuts_draw) : 0, 0);
            if ((stats && hipMemset(d.rec, 0, got_rec.size()) != hipSuccess) ||
                hipMemcpy(d.x, x0.data(), n * D * sizeof(TT), hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(d.ad, ad0.data(), n * sizeof(mm_nuts_adapt<ST>), hipMemcpyHostToDevice) != hipSuccess)
                return false;
            /* run_progress' stepping: all ten transitions, the last five recorded; from step 0 of the probe's own stream */
            mm_nuts_init_args<TT, ST> ia;
            mm_nuts_args<TT, ST> a;
            fill_args(Where{d.x, d.ad, d.out, nullptr, nullptr, d.scratch, n, 0x5eedull, 0, 0, 10, 0.8, false},
                      mm_nuts_step_plan(nc, nd, 1, dim, 0), nd, &ia, &a);
            return unit_init(unit, metric_kind, ia, d.met, stream) == hipSuccess && unit_run(unit, metric_kind, a, which, d.met, stats, d.rec, stream) == hipSuccess &&
                   hipStreamSynchronize(stream) == hipSuccess &&
                   hipMemcpy(got.data(), d.out, got.size() * sizeof(TT), hipMemcpyDeviceToHost) == hipSuccess &&
                   (!stats || hipMemcpy(got_rec.data(), d.rec, got_rec.size(), hipMemcpyDeviceToHost) == hipSuccess);
        };
        std::vector<TT> a, a2, g;
        std::vector<unsigned char> r, r2, rg;
        if (!one(2, a, r) || !one(2, a2, r2))
            return false;
        bool ok = std::memcmp(a.data(), a2.data(), a.size() * sizeof(TT)) == 0 && r == r2;
        int process_hip = 0, built_hip = 0;
        (void)mmcmc_rtc_compiler_info(nullptr, 0, &process_hip, &built_hip);
        const bool referee_trusted = mm_rtc_compiler(unit) == MMCMC_RTC_COMPILER_HIPCC || (process_hip > 0 && process_hip / 100000 >= built_hip / 100000);
        if (ok && referee_trusted) {
            if (!one(0, g, rg))
                return false;
            ok = std::memcmp(a.data(), g.data(), a.size() * sizeof(TT)) == 0 && r == rg;
        }
        std::lock_guard<std::mutex> l(mu);
        verdict[unit] = ok;
        return ok;
    }

    /* the checks of a metric's values and its device image in the tensor type: s, then r (with the inverse: the stop criterion
     * multiplies by r_i), or L, then L^-1, each packed by rows */
    bool metric_image(bool dense, const double *values, std::vector<TT> &image) const
    {
        if (!dense)
            return mm_diag_prepare<TT>(values, (size_t)dim, true, image);
        std::vector<TT> li;
        if (!mm_dense_prepare<TT>(values, (size_t)dim, image, li))
            return false;
        image.insert(image.end(), li.begin(), li.end());
        return true;
    }

    /* mmcmc_nuts_set_metric (dense = false: values = the scales [dim]) and mmcmc_nuts_set_metric_dense (values = L row-major
     * [dim, dim]): every value is checked before anything changes; NULL, through either, removes whichever metric is set and
     * gives the handle its variant back */
    int set_metric(bool dense, const double *values) override
    {
        if (!values) {
            if (met.kind == MM_METRIC_NONE)
                return MMCMC_OK;
            if (recording) { /* the handle goes on recording on the stats unit without a metric, still variant 7 */
                DevGuard g(device);
                if (!ready_stats_unit(MM_METRIC_NONE))
                    return MMCMC_ERR_UNSUPPORTED;
            }
            met.clear(variant);
            if (recording) {
                variant_before_recording = variant;
                variant = mm_metric_variant;
            }
            return MMCMC_OK;
        }
        if (dense && dim < 1)
            return MMCMC_ERR_INVALID_ARG;
        const size_t D = (size_t)dim;
        std::vector<TT> image;
        if (!metric_image(dense, values, image))
            return MMCMC_ERR_INVALID_ARG;
        if (dim > 32)
            return MMCMC_ERR_UNSUPPORTED;
        DevGuard g(device);
        const mm_user_target *&kept = dense ? dense_unit : metric_unit;
        const mm_user_target *unit = kept ? kept : mm_rtc_metric_unit(kind, dim, dense);
        if (!unit)
            return MMCMC_ERR_UNSUPPORTED; /* no run-time compiler (or the unit does not build): nothing changed */
        MM_HIP(hipDeviceSynchronize()); /* behind every queued run: a metric applies from the next transition on */
        if (!unit_verified(unit, dense ? MM_METRIC_DENSE : MM_METRIC_DIAG, false))
            return MMCMC_ERR_UNSUPPORTED;
        if (recording && !ready_stats_unit(dense ? MM_METRIC_DENSE : MM_METRIC_DIAG)) /* the records go on under the new metric */
            return MMCMC_ERR_UNSUPPORTED;
        if (!d_metric) /* room for either kind: a dense metric's two packed factors */
            MM_HIP(hipMalloc((void **)&d_metric, 2 * mm_tri_len(D) * sizeof(TT)));
        MM_HIP(unit_scratch());
        MM_HIP(hipMemcpy(d_metric, image.data(), image.size() * sizeof(TT), hipMemcpyHostToDevice));
        kept = unit;
        const bool first_metric = met.kind == MM_METRIC_NONE;
        if (dense)
            met.commit_dense(values, D, variant);
        else
            met.commit_diag(values, D, variant);
        if (recording && first_metric) /* the variant to return to is the one from before recording, kept by `met` from here on */
            met.variant_before = variant_before_recording;
        return MMCMC_OK;
    }

    /* the stack area of a metric unit's or a stats unit's kernels */
    hipError_t unit_scratch()
    {
        if (d_metric_scratch)
            return hipSuccess;
        size_t stack = 0, tile = 0;
        unit_sizes((size_t)dim, &stack, &tile);
        return hipMalloc((void **)&d_metric_scratch, (n_chains + 63) / 64 * stack);
    }

    /* the stats unit of a metric kind, built and verified (once per unit, type mode and process), or NULL with nothing changed:
     * a dimension above 32, no run-time compiler, a unit that does not build or fails unit_verified */
    const mm_user_target *ready_stats_unit(int metric_kind)
    {
        if (stats_unit[metric_kind])
            return stats_unit[metric_kind];
        if (dim > 32)
            return nullptr;
        const mm_user_target *unit = mm_rtc_stats_unit(kind, dim, metric_kind);
        if (!unit || hipDeviceSynchronize() != hipSuccess || !unit_verified(unit, metric_kind, true))
            return nullptr;
        return stats_unit[metric_kind] = unit;
    }

    /* mmcmc_nuts_set_draw_stats: every check happens before any change */
    int set_draw_stats(bool on) override
    {
        if (on == recording)
            return MMCMC_OK;
        DevGuard g(device);
        if (!on) {
            MM_HIP(hipDeviceSynchronize()); /* behind the run that writes the records */
            (void)hipFree(d_rec);
            d_rec = nullptr;
            rec_capacity = rec_stride = rec_first = rec_rows = 0;
            rec_valid = false;
            recording = false;
            if (met.kind == MM_METRIC_NONE)
                variant = variant_before_recording;
            return MMCMC_OK;
        }
        if (!ready_stats_unit(met.kind))
            return MMCMC_ERR_UNSUPPORTED;
        MM_HIP(unit_scratch());
        recording = true;
        if (met.kind == MM_METRIC_NONE) { /* with a metric the handle is on variant 7 already and `met` keeps the one to return to */
            variant_before_recording = variant;
            variant = mm_metric_variant;
        }
        return MMCMC_OK;
    }

    int draw_stats(mmcmc_nuts_draw *out, int out_is_device, size_t *n_rows) override
    {
        if (!recording || !rec_valid)
            return MMCMC_ERR_SHAPE;
        if (n_rows)
            *n_rows = rec_rows;
        if (!out || rec_rows == 0)
            return MMCMC_OK;
        DevGuard g(device);
        MM_HIP(hipDeviceSynchronize());
        MM_HIP(hipMemcpy2D(out, rec_rows * sizeof(mm_nuts_draw), d_rec + rec_first, rec_stride * sizeof(mm_nuts_draw), rec_rows * sizeof(mm_nuts_draw),
                           n_chains, out_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
        return MMCMC_OK;
    }
    /* the rows of the last run's records that the caller's sample holds (mmcmc_nuts_run_progress: the last n_collect) */
    int draw_stats_window(size_t first, size_t rows) override
    {
        if (!recording || !rec_valid)
            return MMCMC_OK;
        if (first + rows > rec_stride)
            return MMCMC_ERR_SHAPE;
        rec_first = first;
        rec_rows = rows;
        return MMCMC_OK;
    }

    int setup(const mmcmc_target_desc *t, const double *init)
    {
        int n = 0;
        const mm_nuts_entry<TT, ST> *tab = nuts_table<TT, ST>(&n);
        for (int i = 0; i < n; ++i)
            if (tab[i].kind == t->kind && tab[i].dim == t->dim)
                k = &tab[i];
        generic_ok = mm_generic_kind_ok(t->kind) && t->dim >= 1;
        bool builtin_user = false;
        if (t->kind < MM_USER_KIND_BASE && !k && generic_ok && t->dim <= 32 && g_rtc_create_mode != 2) {
            /* a built-in target at a dimension without a compiled instance: its functor compiled into the one-chain-per-lane
             * kernels on first use (hipRTC, mm_rtc_builtin_nuts); NULL keeps the run-time-D kernel */
            DevGuard gb(device);
            user = mm_rtc_builtin_nuts(t->kind, t->dim);
            /* ... and only if the unit has this type mode's init and pair kernels (mm_rtc_nuts_usable) */
            if (user && !mm_rtc_nuts_usable(user, type_mode))
                user = nullptr;
            builtin_user = user != nullptr;
        }
        if (t->kind >= MM_USER_KIND_BASE || builtin_user) {
            if (!builtin_user)
                user = mm_rtc_find(t->kind);
            if (!user)
                return MMCMC_ERR_INVALID_ARG;
            if (mm_rtc_is_model(user) || mm_rtc_is_discrete(user) || (!builtin_user && mm_rtc_is_internal(user)))
                return MMCMC_ERR_UNSUPPORTED; /* a target + proposal model / an integer-state model has no NUTS kernels; a unit
                                                 the library built for itself is not a kind a caller may name */
            if (mm_rtc_dim(user) != t->dim)
                return MMCMC_ERR_SHAPE;
            if (!builtin_user && mm_rtc_data_len(user) && !t->matrix)
                return MMCMC_ERR_INVALID_ARG; /* a kind that carries data: its functor is never run with P.mat == nullptr */
            if (!builtin_user) {
                DevGuard gu(device);
                if (!mm_rtc_nuts_usable(user, type_mode))
                    return MMCMC_ERR_UNSUPPORTED; /* this dimension and precision need more registers than a lane has */
            }
            unit_sizes((size_t)t->dim, &user_stack_bytes, &user_lds);
        } else if (!k && !generic_ok) {
            return MMCMC_ERR_UNSUPPORTED;
        }
        rtc_unit = user;
        if (user && !builtin_user) {
            for (int i = 0; i < 8; ++i) /* P.p[0..8) = the description's params (mm_rtc.hip) */
                P.p[i] = (TT)t->params[i];
            P.mat = nullptr;
        } else if (mm_fill_params<TT>(t->kind, t->params, &P) != 0) {
            return MMCMC_ERR_INVALID_ARG;
        }
        g_pad = (n_chains + 63) / 64 * 64;
        DevGuard g(device);
        const size_t cd = n_chains * (size_t)dim;
        if (t->kind == MMCMC_GAUSSIAN_ND || (user && t->matrix)) {
            const size_t data_len = user && !builtin_user ? mm_rtc_data_len(user) : 0; /* a data kind: its own length */
            std::vector<TT> h(data_len ? data_len : (size_t)dim * dim);
            for (size_t i = 0; i < h.size(); ++i)
                h[i] = (TT)t->matrix[i];
            MM_HIP(hipMalloc((void **)&d_mat, h.size() * sizeof(TT)));
            MM_HIP(hipMemcpy(d_mat, h.data(), h.size() * sizeof(TT), hipMemcpyHostToDevice));
            P.mat = d_mat;
        }
        std::vector<TT> h(cd);
        for (size_t i = 0; i < cd; ++i)
            h[i] = (TT)init[i]; /* Vec<Vec<T>> -> backend float tensor (nuts.rs:411-413) */
        MM_HIP(hipMalloc((void **)&d_state, cd * sizeof(TT)));
        MM_HIP(hipMemcpy(d_state, h.data(), cd * sizeof(TT), hipMemcpyHostToDevice));
        std::vector<mm_nuts_adapt<ST>> ad(n_chains);
        fresh_adapt(ad);
        MM_HIP(hipMalloc((void **)&d_adapt, n_chains * sizeof(mm_nuts_adapt<ST>)));
        MM_HIP(hipMemcpy(d_adapt, ad.data(), n_chains * sizeof(mm_nuts_adapt<ST>), hipMemcpyHostToDevice));
        MM_HIP(hipMalloc((void **)&d_nlf, n_chains * sizeof(unsigned long long)));
        MM_HIP(hipMemset(d_nlf, 0, n_chains * sizeof(unsigned long long)));
        MM_HIP(hipMalloc((void **)&d_hist, (MM_NUTS_JMAX + 1) * sizeof(unsigned int)));
        MM_HIP(hipMemset(d_hist, 0, (MM_NUTS_JMAX + 1) * sizeof(unsigned int)));
        if (k) {
            /* the pending-subtree stack goes to LDS when tile + stack fit comfortably, else to HBM scratch */
            stack_in_lds = (k->tile_bytes_per_wave + k->stack_bytes_per_wave) <= 40 * 1024;
            /* the scratch area also serves the asynchronous-lane kernel when ITS stack (max_depth levels, no tile) is
             * over the LDS limit; max_depth can change after create, so allocate whenever the full stack is */
            if (!stack_in_lds || k->stack_bytes_per_wave + 4096 > 40 * 1024) { /* + the pair kernel's ring of uniforms */
                const size_t waves = (n_chains + 63) / 64;
                MM_HIP(hipMalloc((void **)&d_scratch, waves * k->stack_bytes_per_wave));
            }
        } else if (user) {
            const size_t waves0 = (n_chains + 63) / 64;
            MM_HIP(hipMalloc((void **)&d_scratch, waves0 * user_stack_bytes));
            stack_in_lds = false;
        }
        if (std::is_same<TT, double>::value && std::is_same<ST, double>::value && t->kind == MMCMC_GAUSSIAN_ND) {
            int nl = 0;
            const mm_nuts_lg_entry *lt = mm_nuts_lg_table(&nl);
            for (int i = 0; i < nl; ++i)
                if (lt[i].dim == t->dim)
                    lg = &lt[i];
            if (lg) {
                const size_t waves = (n_chains + 15) / 16;
                c_pad = waves * 16;
                MM_HIP(hipMalloc((void **)&d_lg_scratch, waves * lg->scratch_doubles_per_wave * sizeof(double)));
                MM_HIP(hipMalloc((void **)&d_lg_rec, c_pad * lg->rec_doubles_per_chain * sizeof(double)));
                MM_HIP(hipMemset(d_lg_rec, 0, c_pad * lg->rec_doubles_per_chain * sizeof(double)));
                MM_HIP(hipMalloc((void **)&d_lg_lists, (size_t)MM_LGQ_SHARDS * MM_LGQ_NQ * c_pad * sizeof(unsigned int)));
                MM_HIP(hipMalloc((void **)&d_lg_ctrl, sizeof(mm_lgq_ctrl)));
                hipDeviceProp_t prop;
                MM_HIP(hipGetDeviceProperties(&prop, device));
                n_resident_waves = (unsigned int)prop.multiProcessorCount * 4u; /* one wave per SIMD */
                MM_HIP(hipMalloc((void **)&d_lg_counts, (size_t)kMaxGroups * 2 * (MM_NUTS_JMAX + 1) * sizeof(unsigned int)));
            }
        }
        caps.inst = k != nullptr;
        caps.inst_async = k && k->run_async;
        caps.inst_pair = k && k->run_pair;
        caps.lg = lg != nullptr;
        caps.generic_ok = generic_ok;
        caps.unit = user != nullptr;
        variant = mm_nuts_default_variant(caps);
        MM_HIP(hipStreamCreateWithFlags(&stream, hipStreamDefault));
        MM_HIP(hipEventCreate(&ev0));
        MM_HIP(hipEventCreate(&ev1));
        return MMCMC_OK;
    }

    /* one launch of the persistent scheduler; the kernel reports a stuck queue instead of hanging */
    hipError_t launch_queue(const mm_nuts_lg_args &gq, const mm_nuts_lgq_shape &shape, hipStream_t st)
    {
        ++n_launches_run;
        hipError_t e = lg->run_queue(gq, shape.nw, shape.occ, st);
        if (e != hipSuccess)
            return e;
        mm_lgq_ctrl hc;
        if ((e = hipMemcpyAsync(&hc, d_lg_ctrl, sizeof(hc), hipMemcpyDeviceToHost, st)) != hipSuccess)
            return e;
        if ((e = hipStreamSynchronize(st)) != hipSuccess)
            return e;
        if (mm_tuning_env("MMCMC_LGQ_STATS"))
            fprintf(stderr, "lgq: first level %d units %llu chains %llu (%.2f per unit) leaf iterations %llu idle polls %llu error %u ticks pick %.3g fetch %.3g work %.3g handover %.3g\n",
                    gq.j0, hc.stat_units, hc.stat_chains, (double)hc.stat_chains / (double)(hc.stat_units ? hc.stat_units : 1),
                    hc.stat_leaf_iters, hc.stat_polls, (unsigned int)hc.error, (double)hc.stat_t[0], (double)hc.stat_t[1],
                    (double)hc.stat_t[2], (double)hc.stat_t[3]);
        return (hc.error != 0ull || hc.remaining != 0ull) ? hipErrorLaunchFailure : hipSuccess;
    }
    /* the first compaction level from the handle's depth histogram (mm_nuts_level_from_hist), kept in auto_level once known */
    hipError_t read_level(hipStream_t st)
    {
        unsigned int hh[MM_NUTS_JMAX + 1];
        hipError_t e = hipMemcpyAsync(hh, d_hist, sizeof(hh), hipMemcpyDeviceToHost, st);
        if (e != hipSuccess || (e = hipStreamSynchronize(st)) != hipSuccess)
            return e;
        const int level = mm_nuts_level_from_hist(hh, n_chains, max_depth);
        if (level >= 0)
            auto_level = level;
        return hipSuccess;
    }
    /* variant 3, the persistent scheduler: one launch, or (a fresh handle, mm_nuts_pilot_split) a pilot and the rest */
    hipError_t run_lg_queue(mm_nuts_lg_args g, hipStream_t st)
    {
        g.ctrl = d_lg_ctrl;
        g.slots = d_lg_lists;
        const mm_nuts_lgq_shape shape =
            mm_nuts_lgq_grid((unsigned int)(c_pad / 16), n_resident_waves, lgq_occ, knob("MMCMC_LGQ_OCC"), knob("MMCMC_LGQ_WAVES"));
        if (!compaction_auto) /* the caller fixed the level */
            return launch_queue(g, shape, st);
        /* once the histogram has fixed the level it is kept: no device-to-host copy and no stream synchronisation per run()
         * after that */
        hipError_t e = auto_level < 0 ? read_level(st) : hipSuccess;
        if (e != hipSuccess)
            return e;
        const mm_knob pilot = knob("MMCMC_LGQ_PILOT"), pilot_level = knob("MMCMC_LGQ_PILOT_LEVEL");
        const mm_nuts_pilot_plan plan = mm_nuts_pilot_split({g.m0, g.n_pre, g.n_rec, g.write_initial, g.out_t0}, auto_level >= 0,
                                                            pilot.set ? (unsigned int)pilot.value : mm_nuts_lgq_pilot);
        for (int i = 0; i < plan.n; ++i) {
            const bool is_pilot = plan.n == 2 && i == 0; /* runs at the default level, then the histogram is read */
            const mm_nuts_segment &s = plan.seg[i];
            mm_nuts_lg_args q = g;
            q.m0 = s.m0;
            q.n_pre = s.n_pre;
            q.n_rec = s.n_rec;
            q.write_initial = s.write_initial;
            q.out_t0 = s.out_t0;
            if (is_pilot && pilot_level.set)
                q.j0 = pilot_level.value;
            if (!is_pilot && auto_level >= 0)
                q.j0 = auto_level < max_depth ? auto_level : max_depth;
            if ((e = launch_queue(q, shape, st)) != hipSuccess || (is_pilot && (e = read_level(st)) != hipSuccess))
                return e;
        }
        return hipSuccess;
    }
    /* variant 2, one launch per level and transition: the chain groups of mm_nuts_lg_group_of, each with its own launch
     * sequence on its own stream between a fork and a join on `st` */
    hipError_t run_lg_levels(const mm_nuts_lg_args &g, hipStream_t st)
    {
        const int n_groups = mm_nuts_lg_n_groups(compaction_groups, n_chains, c_pad);
        const mm_nuts_segment run = {g.m0, g.n_pre, g.n_rec, g.write_initial, g.out_t0};
        hipError_t e = hipMemsetAsync(d_lg_counts, 0, (size_t)kMaxGroups * 2 * (MM_NUTS_JMAX + 1) * sizeof(unsigned int), st);
        if (e != hipSuccess)
            return e;
        if (!lg_fork && (e = hipEventCreateWithFlags(&lg_fork, hipEventDisableTiming)) != hipSuccess)
            return e;
        if ((e = hipEventRecord(lg_fork, st)) != hipSuccess)
            return e;
        for (int gi = 0; gi < n_groups; ++gi) {
            if (!lg_streams[gi] && (e = hipStreamCreateWithFlags(&lg_streams[gi], hipStreamNonBlocking)) != hipSuccess)
                return e;
            if (!lg_join[gi] && (e = hipEventCreateWithFlags(&lg_join[gi], hipEventDisableTiming)) != hipSuccess)
                return e;
            const mm_nuts_lg_group grp = mm_nuts_lg_group_of(gi, n_groups, n_chains, c_pad);
            const size_t off = grp.offset;
            mm_nuts_lg_args q = g;
            q.n_chains = grp.n_chains;
            q.c_pad = grp.c_pad;
            q.chain_offset = g.chain_offset + off;
            q.state = g.state + off * (size_t)dim;
            q.adapt = g.adapt + off;
            q.out = g.out ? g.out + off * g.n_total * (size_t)dim : nullptr;
            q.n_leapfrog = g.n_leapfrog ? g.n_leapfrog + off : nullptr;
            q.scratch = d_lg_scratch + grp.w0 * lg->scratch_doubles_per_wave;
            q.rec = d_lg_rec + off * lg->rec_doubles_per_chain;
            q.lists = d_lg_lists + (size_t)MM_NUTS_JMAX * off;
            q.counts = d_lg_counts + (size_t)gi * 2 * (MM_NUTS_JMAX + 1);
            hipStream_t gs = lg_streams[gi];
            if ((e = hipStreamWaitEvent(gs, lg_fork, 0)) != hipSuccess)
                return e;
            for (unsigned int t = 0; t < run.n_pre + run.n_rec && e == hipSuccess; ++t) {
                const mm_nuts_lg_step s = mm_nuts_lg_step_of(run, t);
                q.m = s.m;
                q.write_initial = s.write_initial;
                q.row = s.row;
                e = lg->run_transition(q, gs);
            }
            if (e != hipSuccess)
                return e;
            if ((e = hipEventRecord(lg_join[gi], gs)) != hipSuccess)
                return e;
            if ((e = hipStreamWaitEvent(st, lg_join[gi], 0)) != hipSuccess)
                return e;
        }
        return hipSuccess;
    }
    /* the lane-group launch exists for <double, double> only; the other instantiations never reach it */
    hipError_t run_lg(const mm_nuts_args<TT, ST> &a, hipStream_t st)
    {
        if constexpr (std::is_same<TT, double>::value && std::is_same<ST, double>::value) {
            mm_nuts_lg_args g = shared_nuts_args<mm_nuts_lg_args>(a);
            g.mat = d_mat;
            g.scratch = d_lg_scratch;
            g.rec = d_lg_rec;
            g.c_pad = c_pad;
            g.lists = d_lg_lists;
            g.counts = d_lg_counts;
            g.j0 = compaction_start < max_depth ? compaction_start : max_depth;
            g.j = 0;
            g.m = 0;
            g.row = 0xffffffffu;
            g.ctrl = nullptr;
            g.slots = nullptr;
            const mm_knob patience = knob("MMCMC_LGQ_PATIENCE"), min_unit = knob("MMCMC_LGQ_MIN_UNIT");
            g.patience = patience.set ? (unsigned int)patience.value : mm_nuts_lgq_patience;
            g.min_unit = min_unit.set ? (unsigned int)min_unit.value : mm_nuts_lgq_min_unit;
            switch (mm_nuts_lg_mode(variant, a.n_pre + a.n_rec, n_chains, c_pad)) {
            case MM_NLG_SINGLE:
                return lg->run(g, st);
            case MM_NLG_QUEUE:
                return run_lg_queue(g, st);
            default:
                return run_lg_levels(g, st);
            }
        } else {
            (void)a;
            (void)st;
            return hipErrorInvalidValue;
        }
    }
    hipError_t init_lg(hipStream_t st)
    {
        if constexpr (std::is_same<TT, double>::value && std::is_same<ST, double>::value)
            return lg->init(P, d_state, d_adapt, n_chains, seed, chain_offset, st);
        else
            return hipErrorInvalidValue;
    }

    /* the run of a run-time compiled target: asynchronous lanes with the leaves in pairs (mm_nuts_pair_body; dynamic LDS = the
     * ring of uniforms, stack in the scratch area).  The unit's lanes-in-step kernel (mm_nuts_run_body) is NOT launched: it gave
     * wrong, run-to-run different samples at RosenbrockND(19) / (23) in f64 and a memory fault at StandardNormal(25) in f32,
     * while the same template compiled into the library by hipcc is correct at those dimensions
     * (tools/experiments/repro_nuts_dims.py).  Round 6 (mm_rtc.hip, at g_compiler): it was the hipRTC the process had loaded --
     * PyTorch's bundled one, whose comgr is the 7.0.2 compiler; the system's 7.2 hipRTC emits hipcc's code and is correct, and
     * today's sources compile correctly under both.  The policy stays: the pair kernel passed every comparison under every
     * compiler, and every unit is checked against a second kernel before its first use (rtc_unit_verified) */
    hipError_t run_target_unit(mm_nuts_args<TT, ST> a, hipStream_t st)
    {
        int run_kernel = rtc_run_kernel;
        /* measurement builds: launch the unit's lanes-in-step kernel from an ordinary handle (never inside the unit's check)
         * -- tools/experiments/rtc_lanes_in_step.py asks whether hipRTC still gets that kernel wrong */
        const mm_knob rk = knob("MMCMC_RTC_RUN_KERNEL");
        if (rk.set && g_rtc_create_mode == 0)
            run_kernel = rk.value == 0 ? 0 : 2;
        const unsigned int grid64 = (unsigned int)((n_chains + 63) / 64);
        return run_kernel == 2 ? mm_rtc_launch_nuts(user, type_mode, 2, &a, sizeof(a), grid64, (size_t)MM_NUTS_RING * 64 * sizeof(double), st)
                               : mm_rtc_launch_nuts(user, type_mode, 0, &a, sizeof(a), grid64, user_lds, st); /* dynamic LDS = its output tile */
    }
    /* the run-time-dimension kernels' block: the run's, the store (mm_gen_nuts_vectors(max_depth) vectors of dim elements per
     * chain, lane-interleaved; run() has sized it) */
    mm_gen_nuts_args<TT, ST> generic_args(const mm_nuts_args<TT, ST> &a) const
    {
        auto ga = shared_nuts_args<mm_gen_nuts_args<TT, ST>>(a);
        ga.P = P;
        ga.kind = kind;
        ga.dim = dim;
        ga.store = d_gstore;
        ga.c_pad = g_pad;
        ga.eps_tol = eps_tol;
        return ga;
    }
    /* the unit of a handle with a metric or one that records: the stats unit of the metric kind while recording */
    const mm_user_target *own_unit(mm_nuts_launch path) const
    {
        return path == MM_NLAUNCH_METRIC_UNIT ? metric_unit : path == MM_NLAUNCH_DENSE_UNIT ? dense_unit : stats_unit[path - MM_NLAUNCH_STATS_UNIT];
    }
    /* one launch on the handle's path: init_chain (nuts.rs:528-545, on every run() call) or the run itself */
    hipError_t launch(mm_nuts_launch path, bool init, mm_nuts_init_args<TT, ST> ia, const mm_nuts_args<TT, ST> &a, hipStream_t st)
    {
        switch (path) {
        case MM_NLAUNCH_INST_STEP:
        case MM_NLAUNCH_INST_ASYNC:
        case MM_NLAUNCH_INST_PAIR:
            if (init)
                return k->init(P, d_state, d_adapt, n_chains, seed, chain_offset, st);
            return path == MM_NLAUNCH_INST_PAIR ? k->run_pair(a, st) : path == MM_NLAUNCH_INST_ASYNC ? k->run_async(a, st) : k->run(a, st);
        case MM_NLAUNCH_LG:
            return init ? init_lg(st) : run_lg(a, st);
        case MM_NLAUNCH_GENERIC:
            return launch_generic(generic_args(a), init ? 1 : 0, st);
        case MM_NLAUNCH_TARGET_UNIT:
            return init ? mm_rtc_launch_nuts(user, type_mode, 1, &ia, sizeof(ia), (unsigned int)((n_chains + 63) / 64), 0, st) : run_target_unit(a, st);
        case MM_NLAUNCH_NONE:
            return hipErrorInvalidValue;
        default: /* the metric unit's or the stats unit's pair kernel, its stack in the handle's metric scratch area */
            return init ? unit_init(own_unit(path), met.kind, ia, d_metric, st)
                        : unit_run(own_unit(path), met.kind, a, 2, d_metric, recording, a.n_total ? d_rec : nullptr, st);
        }
    }

    int run(size_t n_collect, size_t n_discard, void *out, int out_is_device, int progress, void *stream_v) override
    {
        const mm_nuts_steps steps = mm_nuts_step_plan(n_collect, n_discard, progress, dim, m);
        if (steps.status != MMCMC_OK)
            return steps.status;
        const mm_nuts_launch path = mm_nuts_launch_path(caps, met.kind, recording, variant);
        if (path == MM_NLAUNCH_NONE) /* no setter leaves a handle on a variant it lacks the kernels of */
            return MMCMC_ERR_STATE;
        const size_t n_rows = steps.n_rows;
        DevGuard g(device);
        hipStream_t st = stream_v ? (hipStream_t)stream_v : stream;
        const size_t out_bytes = n_chains * n_rows * (size_t)dim * sizeof(TT);
        TT *d_out = nullptr;
        /* host output: a device staging buffer, released on every path out of this function */
        struct Staging {
            void *p = nullptr;
            ~Staging()
            {
                if (p)
                    (void)hipFree(p);
            }
        } staging;
        bool staged = false;
        if (out && n_rows > 0) {
            if (out_is_device) {
                d_out = (TT *)out;
            } else {
                MM_HIP(hipMalloc(&staging.p, out_bytes));
                d_out = (TT *)staging.p;
                staged = true;
            }
        }
        n_launches_run = 0;
        if (path == MM_NLAUNCH_GENERIC && (!d_gstore || gstore_depth < max_depth)) {
            (void)hipFree(d_gstore);
            d_gstore = nullptr;
            MM_HIP(hipMalloc((void **)&d_gstore, (size_t)mm_gen_nuts_vectors(max_depth) * (size_t)dim * g_pad * sizeof(TT)));
            gstore_depth = max_depth;
        }
        if (recording) {
            const size_t need = n_chains * n_rows;
            if (need > rec_capacity) {
                MM_HIP(hipDeviceSynchronize()); /* behind a queued run that writes the buffer */
                (void)hipFree(d_rec);
                d_rec = nullptr;
                rec_capacity = 0;
                rec_valid = false;
                MM_HIP(hipMalloc((void **)&d_rec, need * sizeof(mm_nuts_draw)));
                rec_capacity = need;
            }
        }
        /* a metric unit or a stats unit keeps its stack in the handle's metric scratch area */
        const bool own = path >= MM_NLAUNCH_METRIC_UNIT;
        mm_nuts_init_args<TT, ST> ia;
        mm_nuts_args<TT, ST> a;
        fill_args(Where{d_state, d_adapt, d_out, d_nlf, d_hist, own ? d_metric_scratch : d_scratch, n_chains, seed, chain_offset, m, max_depth,
                        target_accept_p, !own && stack_in_lds},
                  steps, n_discard, &ia, &a);
        a.async_batch = (unsigned int)knob("MMCMC_NUTS_ASYNC_BATCH").value; /* tuning aid; no result depends on it */
        hipError_t e = launch(path, true, ia, a, st);
        if (e != hipSuccess)
            return (int)e;
        MM_HIP(hipEventRecord(ev0, st));
        if ((e = launch(path, false, ia, a, st)) != hipSuccess)
            return (int)e;
        MM_HIP(hipEventRecord(ev1, st));
        if (recording) { /* the records of this run, one per row of its sample */
            rec_stride = rec_rows = n_rows;
            rec_first = 0;
            rec_valid = true;
        }
        m += steps.n_pre + steps.n_rec;
        timed = true;
        /* sampling launches of this run: the persistent scheduler counts its own (a fresh handle: a 16-transition pilot plus
         * the rest); every other path reports 1, compaction by launches (one per level and transition) included; kernel_ms is
         * the time on the stream between the first and the last, host gaps of multi-launch runs included */
        timing.n_launches = n_launches_run ? n_launches_run : 1;
        timing.out_bytes = d_out ? out_bytes : 0;
        timing.state_bytes = 2ull * n_chains * dim * sizeof(TT);
        timing.kernel_ms = -1.f;
        if (staged)
            MM_HIP(mm_copy_to_host(out, d_out, out_bytes, device, st));
        return MMCMC_OK;
    }

    int state(void *out) override
    {
        DevGuard g(device);
        MM_HIP(hipDeviceSynchronize());
        MM_HIP(hipMemcpy(out, d_state, n_chains * (size_t)dim * sizeof(TT), hipMemcpyDeviceToHost));
        return MMCMC_OK;
    }
    int adapt_state(double *out) override
    {
        DevGuard g(device);
        MM_HIP(hipDeviceSynchronize());
        std::vector<mm_nuts_adapt<ST>> ad(n_chains);
        MM_HIP(hipMemcpy(ad.data(), d_adapt, n_chains * sizeof(mm_nuts_adapt<ST>), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n_chains; ++i) {
            out[4 * i + 0] = (double)ad[i].epsilon;
            out[4 * i + 1] = (double)ad[i].epsilon_bar;
            out[4 * i + 2] = (double)ad[i].h_bar;
            out[4 * i + 3] = (double)ad[i].mu;
        }
        return MMCMC_OK;
    }
    /* positions [n_chains, dim] of the tensor type, host or device memory (as mmcmc_hmc_set_state).  Each run() starts
     * with init_chain from the state and the adaptation records (nuts.rs:528-545); nothing else derives from them */
    int set_state(const void *x, int is_device, void *stream_v) override
    {
        DevGuard g(device);
        if (is_device) {
            hipPointerAttribute_t attr{};
            if (hipPointerGetAttributes(&attr, x) != hipSuccess) {
                (void)hipGetLastError();
                return MMCMC_ERR_INVALID_ARG;
            }
            if ((attr.type != hipMemoryTypeDevice && !attr.isManaged) || attr.device != device)
                return MMCMC_ERR_INVALID_ARG;
        }
        hipStream_t st = stream_v ? (hipStream_t)stream_v : stream;
        MM_HIP(hipMemcpyAsync(d_state, x, n_chains * (size_t)dim * sizeof(TT),
                              is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
        if (!is_device)
            MM_HIP(hipStreamSynchronize(st));
        return MMCMC_OK;
    }
    /* the inverse of adapt_state: [n_chains, 4] doubles = epsilon, epsilon_bar, h_bar, mu.  Every value finite in the
     * scalar type, epsilon > 0 or exactly the sentinel -1 (no search yet, nuts.rs:415-433); nothing is written otherwise.
     * The lane-group records (d_lg_rec) and the compaction level are not state: every transition writes its record before
     * reading it, and the level never changes a result */
    int set_adapt_state(const double *in) override
    {
        std::vector<mm_nuts_adapt<ST>> ad(n_chains);
        for (size_t i = 0; i < n_chains; ++i) {
            const double *r = in + 4 * i;
            ad[i].epsilon = (ST)r[0];
            ad[i].epsilon_bar = (ST)r[1];
            ad[i].h_bar = (ST)r[2];
            ad[i].mu = (ST)r[3];
            const ST v[4] = {ad[i].epsilon, ad[i].epsilon_bar, ad[i].h_bar, ad[i].mu};
            for (int q = 0; q < 4; ++q)
                if (!std::isfinite(r[q]) || !std::isfinite(v[q]))
                    return MMCMC_ERR_INVALID_ARG;
            if (!(ad[i].epsilon > ST(0)) && r[0] != -1.0)
                return MMCMC_ERR_INVALID_ARG;
        }
        DevGuard g(device);
        MM_HIP(hipDeviceSynchronize()); /* behind every queued run, like adapt_state */
        MM_HIP(hipMemcpy(d_adapt, ad.data(), n_chains * sizeof(mm_nuts_adapt<ST>), hipMemcpyHostToDevice));
        return MMCMC_OK;
    }
    int leapfrog_counts(uint64_t *out) override
    {
        DevGuard g(device);
        MM_HIP(hipDeviceSynchronize());
        MM_HIP(hipMemcpy(out, d_nlf, n_chains * sizeof(uint64_t), hipMemcpyDeviceToHost));
        return MMCMC_OK;
    }
    int depth_histogram(uint32_t *out) override
    {
        DevGuard g(device);
        MM_HIP(hipDeviceSynchronize());
        MM_HIP(hipMemcpy(out, d_hist, (MM_NUTS_JMAX + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
        return MMCMC_OK;
    }
};

} // namespace

struct mmcmc_nuts {
    NutsBase *p;
};

/* A run-time compiled unit is checked once per (unit, type mode) and process before a handle relies on it: 96 chains, 5 + 5
 * transitions from a fixed start, (a) twice -- the two must be the same bits --, (b) against a SECOND, differently built
 * kernel of the same transitions, which must agree bit for bit: for a built-in target the run-time-dimension kernel
 * (variant 6, compiled into the library by hipcc); for a USER target -- whose functor exists only inside its unit -- the
 * unit's own lanes-in-step kernel (mm_nuts_run_body: another control structure around the same functor, the pair the
 * library's compiled instances are tested to agree on, variants 0 and 5) WHEN hipcc built the unit.  Why: tools/experiments/repro_nuts_dims.py found
 * hipRTC-built kernels that do not reproduce themselves or are plainly wrong (the lanes-in-step kernel at RosenbrockND(19)
 * and (23) in f64, StandardNormal(25) in f32) while hipcc builds of the same source are right; units are now built by hipcc
 * where it exists (mm_rtc.hip) and what IS launched is still checked.  A unit that fails leaves a built-in target on the
 * run-time-dimension kernel; a user target is refused.  Only real verdicts are cached: an allocation or launch error
 * inside the check fails this create and is tried again by the next one. */
extern "C" int mmcmc_nuts_create(mmcmc_nuts **out, const mmcmc_target_desc *target, const double *init, size_t n_chains,
                                 double target_accept_p, int mode, int device);
extern "C" int mmcmc_nuts_destroy(mmcmc_nuts *h);
static bool rtc_unit_verified(const void *unit, const mmcmc_target_desc *target, int mode, int device)
{
    static std::mutex mu;
    static std::map<std::pair<const void *, int>, bool> verdict;
    {
        std::lock_guard<std::mutex> l(mu);
        auto it = verdict.find({unit, mode});
        if (it != verdict.end())
            return it->second;
    }
    const size_t n = 96, dim = (size_t)target->dim, nc = 5, nd = 5, esz = mode == 2 ? 8 : 4;
    std::vector<double> x0(n * dim);
    for (size_t c = 0; c < n; ++c)
        for (size_t i = 0; i < dim; ++i)
            x0[c * dim + i] = 0.05 * (double)((int)((c * 7 + i * 13) % 17) - 8);
    bool errored = false;
    /* variant < 0: the handle's default (the unit's pair kernel); rtc_kernel: which run kernel of the unit */
    auto one = [&](int variant, int rtc_kernel, std::vector<unsigned char> &bytes) -> bool {
        mmcmc_nuts *t = nullptr;
        if (mmcmc_nuts_create(&t, target, x0.data(), n, 0.8, mode, device) != MMCMC_OK) {
            errored = true;
            return false;
        }
        bytes.assign(n * nc * dim * esz, 0);
        t->p->seed = 0x5eedull;
        t->p->rtc_run_kernel = rtc_kernel;
        bool ok = (variant < 0 ? t->p->rtc_unit == unit : t->p->set_variant(variant) == MMCMC_OK);
        if (ok && t->p->run(nc, nd, bytes.data(), 0, 1, nullptr) != MMCMC_OK) {
            errored = true;
            ok = false;
        }
        (void)mmcmc_nuts_destroy(t);
        return ok;
    };
    g_rtc_create_mode = 1;
    std::vector<unsigned char> a, a2, g;
    bool ok = one(-1, 2, a) && one(-1, 2, a2) && a == a2;
    /* the second opinion of a USER unit is the unit's lanes-in-step kernel -- the very kernel hipRTC was caught miscompiling
     * (wrong samples at RosenbrockND(19) / (23) f64, a device memory fault at StandardNormal(25) f32): it is launched only
     * from units hipcc built -- and (round 6, when the compiler was identified: the hipRTC PyTorch bundles, ROCm 7.0.2's;
     * the system's 7.2 emits hipcc's code) from units built by the hipRTC of a runtime at least as new as the compiler this
     * library was built with.  A user unit built by an OLDER hipRTC (no hipcc on the machine, torch imported first) keeps
     * the run-twice check alone: refusing a correct pair kernel on the word of a broken referee, or faulting the process
     * inside the check, would be worse than the exposure it closes (advisor r4). */
    int process_hip = 0, built_hip = 0;
    (void)mmcmc_rtc_compiler_info(nullptr, 0, &process_hip, &built_hip);
    const bool referee_trusted = mm_rtc_compiler((const mm_user_target *)unit) == MMCMC_RTC_COMPILER_HIPCC ||
                                 (process_hip > 0 && process_hip / 100000 >= built_hip / 100000);
    if (ok && target->kind < MM_USER_KIND_BASE)
        ok = one(6, 2, g) && a == g;
    else if (ok && referee_trusted)
        ok = one(-1, 0, g) && a == g;
    g_rtc_create_mode = 0;
    if (!errored) {
        std::lock_guard<std::mutex> l(mu);
        verdict[{unit, mode}] = ok;
    }
    return ok;
}

extern "C" {

int mmcmc_nuts_create(mmcmc_nuts **out, const mmcmc_target_desc *target, const double *init, size_t n_chains,
                      double target_accept_p, int mode, int device)
{
    if (!out)
        return MMCMC_ERR_INVALID_ARG;
    *out = nullptr;
    if (!target || !init || n_chains == 0 || target->dim <= 0 || mode < 0 || mode > 2 ||
        !(target_accept_p > 0.0 && target_accept_p < 1.0))
        return MMCMC_ERR_INVALID_ARG;
    if (target->kind == MMCMC_GAUSSIAN_ND && !target->matrix)
        return MMCMC_ERR_INVALID_ARG;
    if ((target->kind == MMCMC_GAUSSIAN2D || target->kind == MMCMC_DIFFABLE_GAUSSIAN2D ||
         target->kind == MMCMC_ROSENBROCK2D) &&
        target->dim != 2)
        return MMCMC_ERR_SHAPE;
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0)
        return MMCMC_ERR_NO_DEVICE;
    if (device < 0 || device >= nd)
        return MMCMC_ERR_INVALID_ARG;
    NutsBase *p = nullptr;
    if (mode == 0)
        p = new (std::nothrow) Nuts<float, double>();
    else if (mode == 1)
        p = new (std::nothrow) Nuts<float, float>();
    else
        p = new (std::nothrow) Nuts<double, double>();
    if (!p)
        return (int)hipErrorOutOfMemory;
    p->device = device;
    p->mode = mode;
    p->kind = target->kind;
    p->dim = target->dim;
    p->n_chains = n_chains;
    p->target_accept_p = target_accept_p;
    int st;
    if (mode == 0)
        st = static_cast<Nuts<float, double> *>(p)->setup(target, init);
    else if (mode == 1)
        st = static_cast<Nuts<float, float> *>(p)->setup(target, init);
    else
        st = static_cast<Nuts<double, double> *>(p)->setup(target, init);
    if (st != MMCMC_OK) {
        delete p;
        return st;
    }
    mmcmc_nuts *h = new (std::nothrow) mmcmc_nuts{p};
    if (!h) {
        delete p;
        return (int)hipErrorOutOfMemory;
    }
    if (p->rtc_unit && g_rtc_create_mode == 0 && !rtc_unit_verified(p->rtc_unit, target, mode, device)) {
        /* the unit's kernels do not reproduce themselves (or the run-time-dimension kernel): not used */
        (void)mmcmc_nuts_destroy(h);
        if (target->kind >= MM_USER_KIND_BASE)
            return MMCMC_ERR_UNSUPPORTED;
        g_rtc_create_mode = 2;
        const int st2 = mmcmc_nuts_create(out, target, init, n_chains, target_accept_p, mode, device);
        g_rtc_create_mode = 0;
        return st2;
    }
    *out = h;
    return MMCMC_OK;
}

int mmcmc_nuts_seed(mmcmc_nuts *h, uint64_t seed)
{
    if (!h)
        return MMCMC_ERR_INVALID_ARG;
    h->p->seed = seed;
    return MMCMC_OK;
}
int mmcmc_nuts_set_chain_offset(mmcmc_nuts *h, uint64_t off)
{
    if (!h)
        return MMCMC_ERR_INVALID_ARG;
    h->p->chain_offset = off;
    return MMCMC_OK;
}
int mmcmc_nuts_set_max_depth(mmcmc_nuts *h, int max_depth)
{
    if (!h || max_depth < 1 || max_depth > MM_NUTS_JMAX)
        return MMCMC_ERR_INVALID_ARG;
    h->p->max_depth = max_depth;
    return MMCMC_OK;
}
int mmcmc_nuts_set_kernel_variant(mmcmc_nuts *h, int variant)
{
    return h ? h->p->set_variant(variant) : MMCMC_ERR_INVALID_ARG;
}
int mmcmc_nuts_kernel_variant(mmcmc_nuts *h) { return h ? h->p->variant : MMCMC_ERR_INVALID_ARG; }
int mmcmc_nuts_set_compaction(mmcmc_nuts *h, int first_level, int n_groups)
{
    if (!h || first_level < 0 || first_level > MM_NUTS_JMAX || n_groups < 0 || n_groups > 16)
        return MMCMC_ERR_INVALID_ARG;
    h->p->compaction_start = first_level;
    h->p->compaction_auto = false;
    h->p->compaction_groups = n_groups;
    return MMCMC_OK;
}
int mmcmc_nuts_run(mmcmc_nuts *h, size_t n_collect, size_t n_discard, void *out, int out_is_device, int progress,
                   void *stream)
{
    return h ? h->p->run(n_collect, n_discard, out, out_is_device, progress, stream) : MMCMC_ERR_INVALID_ARG;
}
int mmcmc_nuts_shape(mmcmc_nuts *h, size_t *n_chains, int *dim, int *mode, int *device)
{
    if (!h)
        return MMCMC_ERR_INVALID_ARG;
    if (n_chains)
        *n_chains = h->p->n_chains;
    if (dim)
        *dim = h->p->dim;
    if (mode)
        *mode = h->p->mode;
    if (device)
        *device = h->p->device;
    return MMCMC_OK;
}
int mmcmc_nuts_state(mmcmc_nuts *h, void *out) { return (h && out) ? h->p->state(out) : MMCMC_ERR_INVALID_ARG; }
int mmcmc_nuts_adapt_state(mmcmc_nuts *h, double *out)
{
    return (h && out) ? h->p->adapt_state(out) : MMCMC_ERR_INVALID_ARG;
}
int mmcmc_nuts_set_metric(mmcmc_nuts *h, const double *scale) { return h ? h->p->set_metric(false, scale) : MMCMC_ERR_INVALID_ARG; }
int mmcmc_nuts_metric(mmcmc_nuts *h, double *scale_out)
{
    return h && scale_out ? h->p->met.report_scale(scale_out, (size_t)h->p->dim) : MMCMC_ERR_INVALID_ARG;
}
int mmcmc_nuts_set_metric_dense(mmcmc_nuts *h, const double *chol) { return h ? h->p->set_metric(true, chol) : MMCMC_ERR_INVALID_ARG; }
int mmcmc_nuts_metric_dense(mmcmc_nuts *h, double *chol_out) { return h && chol_out ? h->p->met.report_chol(chol_out) : MMCMC_ERR_INVALID_ARG; }
int mmcmc_nuts_set_draw_stats(mmcmc_nuts *h, int on) { return h ? h->p->set_draw_stats(on != 0) : MMCMC_ERR_INVALID_ARG; }
int mmcmc_nuts_draw_stats_enabled(mmcmc_nuts *h) { return h ? (h->p->recording ? 1 : 0) : MMCMC_ERR_INVALID_ARG; }
int mmcmc_nuts_draw_stats(mmcmc_nuts *h, mmcmc_nuts_draw *out, int out_is_device, size_t *n_rows)
{
    return h ? h->p->draw_stats(out, out_is_device, n_rows) : MMCMC_ERR_INVALID_ARG;
}
int mmcmc_nuts_set_state(mmcmc_nuts *h, const void *x, int is_device, void *stream)
{
    return (h && x) ? h->p->set_state(x, is_device, stream) : MMCMC_ERR_INVALID_ARG;
}
int mmcmc_nuts_set_adapt_state(mmcmc_nuts *h, const double *in)
{
    return (h && in) ? h->p->set_adapt_state(in) : MMCMC_ERR_INVALID_ARG;
}
/* target_accept_p (fixed by mmcmc_nuts_create) and max_depth (mmcmc_nuts_set_max_depth); either pointer may be NULL */
int mmcmc_nuts_params(mmcmc_nuts *h, double *target_accept_p, int *max_depth)
{
    if (!h)
        return MMCMC_ERR_INVALID_ARG;
    if (target_accept_p)
        *target_accept_p = h->p->target_accept_p;
    if (max_depth)
        *max_depth = h->p->max_depth;
    return MMCMC_OK;
}
int mmcmc_nuts_set_target_accept_p(mmcmc_nuts *h, double target_accept_p)
{
    if (!h || !(target_accept_p > 0.0 && target_accept_p < 1.0)) /* mmcmc_nuts_create's check */
        return MMCMC_ERR_INVALID_ARG;
    h->p->target_accept_p = target_accept_p;
    return MMCMC_OK;
}
int mmcmc_nuts_stream_position(mmcmc_nuts *h, uint64_t *seed, uint64_t *chain_offset, uint64_t *iteration)
{
    if (!h)
        return MMCMC_ERR_INVALID_ARG;
    if (seed)
        *seed = h->p->seed;
    if (chain_offset)
        *chain_offset = h->p->chain_offset;
    if (iteration)
        *iteration = h->p->m;
    return MMCMC_OK;
}
/* self.m: the transitions taken so far -- it keys the noise and, against n_discard, the adaptation (nuts.rs:682) */
int mmcmc_nuts_set_iteration(mmcmc_nuts *h, uint64_t iteration)
{
    if (!h || iteration >= (1ull << 32))
        return MMCMC_ERR_INVALID_ARG;
    h->p->m = (uint32_t)iteration;
    return MMCMC_OK;
}
int mmcmc_nuts_leapfrog_counts(mmcmc_nuts *h, uint64_t *out)
{
    return (h && out) ? h->p->leapfrog_counts(out) : MMCMC_ERR_INVALID_ARG;
}
int mmcmc_nuts_depth_histogram(mmcmc_nuts *h, uint32_t *out)
{
    return (h && out) ? h->p->depth_histogram(out) : MMCMC_ERR_INVALID_ARG;
}
int mmcmc_nuts_sync(mmcmc_nuts *h)
{
    if (!h)
        return MMCMC_ERR_INVALID_ARG;
    DevGuard g(h->p->device);
    MM_HIP(hipStreamSynchronize(h->p->stream));
    return MMCMC_OK;
}
int mmcmc_nuts_timing(mmcmc_nuts *h, mmcmc_timing *t)
{
    if (!h || !t)
        return MMCMC_ERR_INVALID_ARG;
    if (!h->p->timed)
        return MMCMC_ERR_STATE;
    DevGuard g(h->p->device);
    MM_HIP(hipEventSynchronize(h->p->ev1));
    float ms = 0.f;
    MM_HIP(hipEventElapsedTime(&ms, h->p->ev0, h->p->ev1));
    h->p->timing.kernel_ms = ms;
    *t = h->p->timing;
    return MMCMC_OK;
}
int mmcmc_nuts_destroy(mmcmc_nuts *h)
{
    if (!h)
        return MMCMC_ERR_INVALID_ARG;
    delete h->p;
    delete h;
    return MMCMC_OK;
}

} /* extern "C" */

int mm_nuts_draw_stats_window(mmcmc_nuts *h, size_t first_row, size_t n_rows) { return h ? h->p->draw_stats_window(first_row, n_rows) : MMCMC_ERR_INVALID_ARG; }
