/*
 * mm_api.hip -- implementation of the C ABI in include/mmcmc.h (MH, HMC, densities, init).
 *
 * Host logic only: handles, argument checking, kernel lookup, launches, timing.  All arithmetic of the hot path
 * lives in mm_samplers.h / mm_targets.h / mm_rng.h and runs on the device; nothing here computes a transition
 * on the CPU and nothing here touches oracle/.
 */
#include "../../include/mmcmc.h"
#include "mm_host.h"
#include "mm_metric_host.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <type_traits>
#include <tuple>
#include <vector>

#include "mm_generic.h"
#include "mm_hmc_lg.h"
#include "mm_hostcopy.h"
#include "mm_kernels.h"
#include "mm_host_rng.h"
#include "mm_params.h"
#include "mm_path.h"
#include "mm_wide.h"
#include "mm_tuning.h"
#include "mm_rtc.h"

size_t mm_split_lds_bytes_f32(int dim, int mh); /* mm_inst_f32.hip */

namespace {

template <class T> const mm_kernel_entry<T> *table(int *n);
template <> const mm_kernel_entry<float> *table<float>(int *n) { return mm_kernel_table_f32(n); }
template <> const mm_kernel_entry<double> *table<double>(int *n) { return mm_kernel_table_f64(n); }
template <class T> const mm_noise_entry<T> *noise_table(int *n);
template <> const mm_noise_entry<float> *noise_table<float>(int *n) { return mm_noise_table_f32(n); }
template <> const mm_noise_entry<double> *noise_table<double>(int *n) { return mm_noise_table_f64(n); }

template <class T> const mm_kernel_entry<T> *find_kernel(int kind, int dim)
{
    int n = 0;
    const mm_kernel_entry<T> *t = table<T>(&n);
    for (int i = 0; i < n; ++i)
        if (t[i].kind == kind && t[i].dim == dim)
            return &t[i];
    return nullptr;
}

/* set by mmcmc_mh_create while it creates the sampler of a target + proposal model */
static thread_local bool g_allow_model = false;

int validate_target(const mmcmc_target_desc *t)
{
    if (!t || t->dim <= 0)
        return MMCMC_ERR_INVALID_ARG;
    switch (t->kind) {
    case MMCMC_GAUSSIAN2D:
    case MMCMC_DIFFABLE_GAUSSIAN2D:
    case MMCMC_ROSENBROCK2D:
        if (t->dim != 2)
            return MMCMC_ERR_SHAPE;
        break;
    case MMCMC_ISOTROPIC_GAUSSIAN:
        if (!(t->params[0] > 0.0))
            return MMCMC_ERR_INVALID_ARG;
        break;
    case MMCMC_ROSENBROCK_ND:
    case MMCMC_STANDARD_NORMAL:
        break;
    case MMCMC_GAUSSIAN_ND:
        if (!t->matrix)
            return MMCMC_ERR_INVALID_ARG;
        break;
    default: {
        /* a kind handed out by mmcmc_target_register_source (mm_rtc.hip) */
        const mm_user_target *u = mm_rtc_find(t->kind);
        if (!u)
            return MMCMC_ERR_UNSUPPORTED;
        if (mm_rtc_is_internal(u))
            return MMCMC_ERR_UNSUPPORTED; /* a unit the library built for itself is not a kind a caller may name */
        if (mm_rtc_dim(u) != t->dim)
            return MMCMC_ERR_SHAPE;
        /* a target + proposal model (mmcmc_proposal_register_source) is reached through mmcmc_mh_create's proposal
         * description only, which checks its base target itself */
        if (mm_rtc_is_model(u) && !g_allow_model)
            return MMCMC_ERR_UNSUPPORTED;
        if (mm_rtc_is_discrete(u))
            return MMCMC_ERR_UNSUPPORTED; /* an integer-state model belongs to mmcmc_mh_discrete_create */
        if (mm_rtc_is_model(u) && mm_rtc_base_kind(u) == MMCMC_GAUSSIAN_ND && !t->matrix)
            return MMCMC_ERR_INVALID_ARG;
        if (mm_rtc_data_len(u) && !t->matrix)
            return MMCMC_ERR_INVALID_ARG; /* a kind that carries data: its functor is never run with P.mat == nullptr */
        break;
    }
    }
    return MMCMC_OK;
}

/* device-side parameter block in element type T (mm_params.h) + the GaussianND matrix uploaded to HBM */
template <class T> int make_params(const mmcmc_target_desc *t, mm_tparams<T> *P, T **d_mat)
{
    *d_mat = nullptr;
    /* a model over a BUILT-IN target derives its parameter block like that target (Sigma^-1, 1 / sigma^2, ...) */
    const int base = t->kind >= MM_USER_KIND_BASE ? mm_rtc_base_kind(mm_rtc_find(t->kind)) : t->kind;
    if (t->kind >= MM_USER_KIND_BASE && !(base >= 0 && base < MM_USER_KIND_BASE)) {
        /* user target: the description's parameters as they are; `matrix`, if given, is dim x dim -- or, for a kind registered
         * with its data (mmcmc_target_register_data_source), that kind's data_len */
        std::memset(P, 0, sizeof *P);
        for (int i = 0; i < 8; ++i)
            P->p[i] = (T)t->params[i];
    } else if (mm_fill_params<T>(base, t->params, P) != 0)
        return MMCMC_ERR_INVALID_ARG;
    if (t->kind == MMCMC_GAUSSIAN_ND || (t->kind >= MM_USER_KIND_BASE && t->matrix)) {
        size_t n = (size_t)t->dim * t->dim;
        if (t->kind >= MM_USER_KIND_BASE)
            if (const size_t data_len = mm_rtc_data_len(mm_rtc_find(t->kind)))
                n = data_len;
        std::vector<T> h(n);
        for (size_t i = 0; i < n; ++i)
            h[i] = (T)t->matrix[i];
        MM_HIP(hipMalloc((void **)d_mat, n * sizeof(T)));
        MM_HIP(hipMemcpy(*d_mat, h.data(), n * sizeof(T), hipMemcpyHostToDevice));
        P->mat = *d_mat;
    }
    return MMCMC_OK;
}

/* one sampler handle; MH and HMC differ only in the kernel entry and two scalars */
struct Sampler {
    int sampler = 0; /* MM_SAMPLER_MH / MM_SAMPLER_HMC */
    int dtype = MMCMC_F32;
    int device = 0;
    int kind = 0, dim = 0;
    size_t n_chains = 0;
    double scale = 0; /* proposal std or step size */
    int n_leapfrog = 0;
    uint64_t seed = 0, chain_offset = 0;
    uint64_t iter = 0;
    uint32_t iters_per_launch = 0;
    mm_path_caps caps;        /* what decides the kernel path (mm_path.h), gathered once by sampler_create */
    int variant = MM_VAR_PAIRED; /* MM_VAR_* (mm_path.h): 0 plain; 1 alias of 2; 2 paired + pipelined noise; 3 lane groups + MFMA
                                    (HMC, GaussianND of dim 16 / 32); 5 noise waves + transition waves (up to dim 8, the f32
                                    default); 6 run-time dimension; 7 run-time compiled unit; 8 wide (HMC, one chain per
                                    workgroup).  Always one mm_variant_status allows; the default is mm_default_variant's */
    const mm_user_target *user = nullptr; /* the run-time compiled unit (mm_rtc.hip) when caps.unit says there is one */
    void *d_gscratch = nullptr; /* the run-time-dimension path's HBM store when the chain vectors do not fit LDS */
    void *d_stage = nullptr;    /* device staging of a sample that goes to the host (sampler_run) */
    size_t stage_cap = 0;
    size_t c_pad = 0;
    unsigned int block = 64;
    void *d_state = nullptr;
    void *d_mat = nullptr;
    unsigned long long *d_accept = nullptr;
    unsigned long long *d_accept_total = nullptr;
    mm_tparams<float> Pf;
    mm_tparams<double> Pd;
    const mm_kernel_entry<float> *kf = nullptr;
    const mm_kernel_entry<double> *kd = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    bool want_accept = true; /* this run(): per-chain accept counts requested */
    bool timing_enabled = true;
    mmcmc_timing timing{};
    /* scheduled runs (mmcmc_hmc_run_scheduled): the device schedule [n + 1] of mm_sched_step<T>, grown on demand, its host
     * image, and an event after the last run that read them (both are rewritten only once it has passed) */
    void *d_sched = nullptr;
    size_t sched_cap = 0;
    std::vector<unsigned char> h_sched;
    hipEvent_t ev_sched = nullptr;
    bool sched_pending = false;
    /* set for the duration of a scheduled run whose variant has a scheduled kernel: launch_range launches it */
    const void *sched_run = nullptr;
    uint32_t sched_iter0 = 0;
    /* HMC's metric (mmcmc_hmc_set_metric, _set_metric_dense): the record of what is set (mm_metric_host.h; caps.metric and
     * caps.dense follow its kind, sync_metric_caps), the device image in the handle's element type -- s [dim], or L packed by
     * rows; room for either --, and the diagonal and the dense unit whose kernels read it */
    mm_metric_record met;
    void *d_metric = nullptr;
    const mm_user_target *metric_unit = nullptr, *dense_unit = nullptr;

    size_t esize() const { return dtype == MMCMC_F32 ? 4 : 8; }
};
static_assert(MM_VAR_UNIT == mm_metric_variant, "a handle with a metric is on its metric unit");

/* the one place where the path rule's two metric facts are assigned */
void sync_metric_caps(Sampler *s)
{
    s->caps.metric = s->met.kind != MM_METRIC_NONE;
    s->caps.dense = s->met.kind == MM_METRIC_DENSE;
}

int sampler_create(Sampler **out, int sampler, const mmcmc_target_desc *target, double scale, int n_leapfrog,
                   const void *init, size_t n_chains, int dtype, int device);
int sampler_destroy(Sampler *s);
int sampler_run(Sampler *s, size_t n_collect, size_t n_discard, void *out, int out_is_device, uint64_t *accept_counts,
                void *stream_v, size_t n_total_rows = 0, size_t row0 = 0, const double *sched_eps = nullptr,
                const int32_t *sched_L = nullptr);

thread_local bool g_in_unit_check = false;

/* A built-in target's run-time compiled MH / HMC unit (mm_rtc_builtin, variant 7) is checked once per (unit, sampler,
 * dtype) and process before a handle relies on it, like the NUTS units (mm_nuts_api.hip): 96 chains, 5 + 5 transitions from
 * a fixed start, run twice -- the same bits -- and against the run-time-dimension kernel (variant 6), bit for bit.  The
 * compiler that builds these units was caught miscompiling a sibling kernel, and a miscompiled unit would
 * otherwise return wrong samples silently.  Only real verdicts are cached: a failed allocation or launch inside the check
 * leaves this handle on variant 6 and is tried again by the next one. */
bool builtin_unit_verified(const mm_user_target *unit, int sampler, const mmcmc_target_desc *target, int dtype, int device)
{
    static std::mutex mu;
    static std::map<std::tuple<const void *, int, int>, bool> verdict;
    const auto key = std::make_tuple((const void *)unit, sampler, dtype);
    {
        std::lock_guard<std::mutex> l(mu);
        auto it = verdict.find(key);
        if (it != verdict.end())
            return it->second;
    }
    const size_t n = 96, dim = (size_t)target->dim, nc = 5, nd = 5, esz = dtype == MMCMC_F32 ? 4 : 8;
    std::vector<unsigned char> x0(n * dim * esz);
    for (size_t c = 0; c < n; ++c)
        for (size_t i = 0; i < dim; ++i) {
            const double v = 0.05 * (double)((int)((c * 7 + i * 13) % 17) - 8);
            if (dtype == MMCMC_F32)
                ((float *)x0.data())[c * dim + i] = (float)v;
            else
                ((double *)x0.data())[c * dim + i] = v;
        }
    bool errored = false;
    auto one = [&](int variant, std::vector<unsigned char> &bytes) -> bool {
        Sampler *t = nullptr;
        /* modest fixed scales: the check is about the kernels, not about the caller's tuning */
        if (sampler_create(&t, sampler, target, sampler == MM_SAMPLER_HMC ? 0.01 : 0.25, sampler == MM_SAMPLER_HMC ? 3 : 0,
                           x0.data(), n, dtype, device) != MMCMC_OK) {
            errored = true;
            return false;
        }
        bytes.assign(n * nc * dim * esz, 0);
        t->seed = 0x5eedull;
        bool ok = t->user == unit; /* the nested handle must be on this very unit */
        if (ok)
            t->variant = variant;
        if (ok && sampler_run(t, nc, nd, bytes.data(), 0, nullptr, nullptr, 0, 0) != MMCMC_OK) {
            errored = true;
            ok = false;
        }
        (void)sampler_destroy(t);
        return ok;
    };
    g_in_unit_check = true;
    std::vector<unsigned char> a, a2, g;
    const bool ok = one(7, a) && one(7, a2) && one(6, g) && a == a2 && a == g;
    g_in_unit_check = false;
    if (!errored) {
        std::lock_guard<std::mutex> l(mu);
        verdict[key] = ok;
    }
    return ok;
}

int sampler_create(Sampler **out, int sampler, const mmcmc_target_desc *target, double scale, int n_leapfrog,
                   const void *init, size_t n_chains, int dtype, int device)
{
    if (!out)
        return MMCMC_ERR_INVALID_ARG;
    *out = nullptr;
    if (!init || n_chains == 0 || (dtype != MMCMC_F32 && dtype != MMCMC_F64) || !(scale > 0.0) ||
        !std::isfinite(scale) || n_leapfrog < 0)
        return MMCMC_ERR_INVALID_ARG;
    int st = validate_target(target);
    if (st != MMCMC_OK)
        return st;
    st = mm_check_device(device);
    if (st != MMCMC_OK)
        return st;
    Sampler *s = new (std::nothrow) Sampler();
    if (!s)
        return (int)hipErrorOutOfMemory;
    s->sampler = sampler;
    s->dtype = dtype;
    s->device = device;
    s->kind = target->kind;
    s->dim = target->dim;
    s->n_chains = n_chains;
    s->scale = scale;
    s->n_leapfrog = n_leapfrog;
    mm_path_caps &c = s->caps;
    c.sampler = sampler;
    c.dtype = dtype;
    c.dim = s->dim;
    auto entry_caps = [&c](const auto *k) {
        c.fixed = k != nullptr;
        c.split = k && k->run_mh_split && k->run_hmc_split && k->run_hmc_split10;
        c.pp_sched = k && k->run_hmc_pp_sched;
        c.split_sched = c.split && k->run_hmc_split_sched;
    };
    if (dtype == MMCMC_F32)
        entry_caps(s->kf = find_kernel<float>(s->kind, s->dim));
    else
        entry_caps(s->kd = find_kernel<double>(s->kind, s->dim));
    c.generic_ok = mm_generic_kind_ok(s->kind);
    /* the run-time-dimension path keeps a chain's vectors in LDS when they fit */
    c.generic_lds = c.generic_ok && (dtype == MMCMC_F32 ? mm_generic_store_bytes<float>(sampler, s->dim)
                                                        : mm_generic_store_bytes<double>(sampler, s->dim)) <= MM_GENERIC_LDS_MAX;
    s->user = s->kind >= MM_USER_KIND_BASE ? mm_rtc_find(s->kind) : nullptr;
    if (s->user) {
        c.unit = MM_UNIT_CALLER;
    } else if (!c.fixed) {
        /* a dimension without a register-resident kernel: the run-time-dimension path */
        if (!c.generic_ok) {
            delete s;
            return MMCMC_ERR_UNSUPPORTED;
        }
        /* up to dimension 32 the target's own functor is compiled into the register-resident skeletons on first use
         * (hipRTC, mm_rtc_builtin): variant 7 then, with the run-time-D kernel (6) still selectable */
        if (s->dim <= 32) {
            DevGuard gb(device);
            s->user = mm_rtc_builtin(s->kind, s->dim);
            if (s->user)
                c.unit = MM_UNIT_BUILTIN;
        }
    }
    /* dense Gaussian at dim 16 / 32 under HMC (f64 and f32): the lane-group / MFMA kernels, and the default there */
    c.lg_ok = sampler == MM_SAMPLER_HMC && s->kind == MMCMC_GAUSSIAN_ND && (s->dim == 16 || s->dim == 32);
    /* few chains of a huge dimension (hmc.rs:882-916: 6 x 10 000): the coordinates of a chain across a workgroup */
    c.wide_ok = sampler == MM_SAMPLER_HMC && !s->user && mm_wide_kind_ok(s->kind) && s->dim >= 4 && s->dim <= MM_WIDE_MAX_DIM;
    c.few_chains = s->dim >= 128 && n_chains < 1024;
    s->variant = mm_default_variant(c);
    DevGuard g(device);
    auto fail = [&](int code) {
        if (s->d_state)
            (void)hipFree(s->d_state);
        if (s->d_mat)
            (void)hipFree(s->d_mat);
        if (s->d_accept)
            (void)hipFree(s->d_accept);
        if (s->d_accept_total)
            (void)hipFree(s->d_accept_total);
        if (s->d_gscratch)
            (void)hipFree(s->d_gscratch);
        if (s->stream)
            (void)hipStreamDestroy(s->stream);
        if (s->ev0)
            (void)hipEventDestroy(s->ev0);
        if (s->ev1)
            (void)hipEventDestroy(s->ev1);
        delete s;
        return code;
    };
    if (dtype == MMCMC_F32) {
        float *m = nullptr;
        st = make_params<float>(target, &s->Pf, &m);
        s->d_mat = m;
    } else {
        double *m = nullptr;
        st = make_params<double>(target, &s->Pd, &m);
        s->d_mat = m;
    }
    if (st != MMCMC_OK)
        return fail(st);
    size_t bytes = n_chains * (size_t)s->dim * s->esize();
    hipError_t e;
    if ((e = hipMalloc(&s->d_state, bytes)) != hipSuccess)
        return fail((int)e);
    if ((e = hipMemcpy(s->d_state, init, bytes, hipMemcpyHostToDevice)) != hipSuccess)
        return fail((int)e);
    s->c_pad = (n_chains + 63) / 64 * 64;
    if (mm_path_generic(c) && !c.generic_lds) {
        /* the run-time-dimension path (default without a fixed-dimension kernel, selectable as variant 6 otherwise)
         * keeps a chain's vectors in LDS when they fit, else in this lane-interleaved HBM store */
        const size_t nvec = sampler == MM_SAMPLER_HMC ? MM_GV_HMC : MM_GV_MH;
        if ((e = hipMalloc(&s->d_gscratch, nvec * (size_t)s->dim * s->c_pad * s->esize())) != hipSuccess)
            return fail((int)e);
    }
    if ((e = hipMalloc((void **)&s->d_accept, n_chains * sizeof(unsigned long long))) != hipSuccess)
        return fail((int)e);
    if ((e = hipMalloc((void **)&s->d_accept_total, sizeof(unsigned long long))) != hipSuccess)
        return fail((int)e);
    if ((e = hipMemset(s->d_accept_total, 0, sizeof(unsigned long long))) != hipSuccess)
        return fail((int)e);
    if ((e = hipStreamCreateWithFlags(&s->stream, hipStreamDefault)) != hipSuccess)
        return fail((int)e);
    if ((e = hipEventCreate(&s->ev0)) != hipSuccess)
        return fail((int)e);
    if ((e = hipEventCreate(&s->ev1)) != hipSuccess)
        return fail((int)e);
    if (c.unit == MM_UNIT_BUILTIN && !g_in_unit_check && !builtin_unit_verified(s->user, sampler, target, dtype, device)) {
        s->user = nullptr; /* the run-time-dimension kernel only (set_kernel_variant(7) is refused then) */
        c.unit = MM_UNIT_NONE;
        s->variant = MM_VAR_GENERIC;
    }
    *out = s;
    return MMCMC_OK;
}

int sampler_destroy(Sampler *s)
{
    if (!s)
        return MMCMC_ERR_INVALID_ARG;
    DevGuard g(s->device);
    (void)hipStreamSynchronize(s->stream);
    (void)hipFree(s->d_state);
    if (s->d_mat)
        (void)hipFree(s->d_mat);
    (void)hipFree(s->d_accept);
    (void)hipFree(s->d_accept_total);
    if (s->d_gscratch)
        (void)hipFree(s->d_gscratch);
    if (s->d_stage)
        (void)hipFree(s->d_stage);
    if (s->d_sched)
        (void)hipFree(s->d_sched);
    if (s->d_metric)
        (void)hipFree(s->d_metric);
    if (s->ev_sched)
        (void)hipEventDestroy(s->ev_sched);
    (void)hipEventDestroy(s->ev0);
    (void)hipEventDestroy(s->ev1);
    (void)hipStreamDestroy(s->stream);
    delete s;
    return MMCMC_OK;
}

/* mm_tile<T, D>::lds_bytes_table + lds_bytes_per_wave for a dimension known only at run time (one wave per workgroup), by
 * the functions mm_kernels.h defines mm_tile through */
static size_t mm_tile_lds_bytes_rt(size_t esz, int D)
{
    return mm_tile_lds_bytes_table(esz) + mm_tile_lds_bytes_per_wave(esz, D, mm_tile_default_t(esz, D));
}
static_assert(mm_tile_lds_bytes_table(4) + mm_tile_lds_bytes_per_wave(4, 3, mm_tile_default_t(4, 3)) ==
                      mm_tile<float, 3>::lds_bytes_table + mm_tile<float, 3>::lds_bytes_per_wave &&
                  mm_tile_lds_bytes_per_wave(8, 9, mm_tile_default_t(8, 9)) == mm_tile<double, 9>::lds_bytes_per_wave &&
                  mm_tile_lds_bytes_per_wave(4, 32, mm_tile_default_t(4, 32)) == mm_tile<float, 32>::lds_bytes_per_wave &&
                  mm_tile<float, 3>::lds_bytes_per_wave == 25600 && mm_tile<double, 32>::lds_bytes_per_wave == 17408,
              "the run-time tile rule is the templates'");

/* the fields every kernel argument struct has under the same name, from the run's mm_run_args */
template <class Q, class T> Q shared_args(const mm_run_args<T> &a)
{
    Q q;
    q.state = a.state;
    q.out = a.out;
    q.accept = a.accept;
    q.accept_total = a.accept_total;
    q.n_chains = a.n_chains;
    q.seed = a.seed;
    q.chain_offset = a.chain_offset;
    q.n_total = a.n_total;
    q.iter0 = a.iter0;
    q.n_discard = a.n_discard;
    q.n_collect = a.n_collect;
    q.out_t0 = a.out_t0;
    return q;
}

template <class T>
int launch_range(Sampler *s, const mm_kernel_entry<T> *k, const mm_tparams<T> &P, T *d_out, size_t n_total,
                 uint32_t n_discard, uint32_t n_collect, uint32_t out_t0, hipStream_t stream)
{
    mm_run_args<T> a;
    a.P = P;
    a.scale = (T)s->scale;
    a.n_leapfrog = s->n_leapfrog;
    a.state = (T *)s->d_state;
    a.out = d_out;
    a.accept = s->want_accept ? s->d_accept : nullptr;
    a.accept_total = s->d_accept_total;
    a.n_chains = s->n_chains;
    a.seed = s->seed;
    a.chain_offset = s->chain_offset;
    a.iter0 = (unsigned int)s->iter;
    a.n_discard = n_discard;
    a.n_collect = n_collect;
    a.out_t0 = out_t0;
    a.n_total = n_total;
    const unsigned int grid = (unsigned int)((s->n_chains + s->block - 1) / s->block);
    hipError_t e = hipErrorNotFound;
    const bool mh = s->sampler == MM_SAMPLER_MH, l10 = s->n_leapfrog == 10;
    const mm_sched_step<T> *sched = (const mm_sched_step<T> *)s->sched_run;
    switch (mm_launch_path(s->caps, s->variant, s->n_leapfrog, sched != nullptr)) {
    case MM_LAUNCH_PLAIN:
        e = mh ? k->run_mh(a, grid, s->block, stream) : k->run_hmc(a, grid, s->block, stream);
        break;
    case MM_LAUNCH_PP:
        e = mh ? k->run_mh_pp(a, grid, s->block, stream) : k->run_hmc_pp(a, grid, s->block, stream);
        break;
    case MM_LAUNCH_PP10:
        e = k->run_hmc_pp10(a, grid, s->block, stream);
        break;
    case MM_LAUNCH_SPLIT:
        e = mh ? k->run_mh_split(a, stream) : k->run_hmc_split(a, stream);
        break;
    case MM_LAUNCH_SPLIT10:
        e = k->run_hmc_split10(a, stream);
        break;
    /* a scheduled run on a variant with a scheduled kernel: (eps, L) per transition from the device */
    case MM_LAUNCH_PP_SCHED:
        e = k->run_hmc_pp_sched(a, sched, s->sched_iter0, grid, s->block, stream);
        break;
    case MM_LAUNCH_SPLIT_SCHED:
        e = k->run_hmc_split_sched(a, sched, s->sched_iter0, stream);
        break;
    case MM_LAUNCH_UNIT: {
        /* the same skeleton (mm_run_kernel_body, PIPE = 2) around the user's functor, from the run-time compiled module */
        /* f32 up to dim 8: the split-role skeleton (four waves per SIMD) where the module has it; else PIPE = 2, one wave per SIMD */
        const char *us = mm_tuning_env("MMCMC_USER_SPLIT"); /* measurement aid: "0" keeps the one-wave-per-SIMD skeleton */
        if (std::is_same<T, float>::value && s->dim <= 8 && !(us && us[0] == '0')) {
            const size_t lds_split = mm_split_lds_bytes_f32(s->dim, mh ? 1 : 0);
            if (lds_split)
                e = mm_rtc_launch_run_split(s->user, mh ? 0 : (l10 ? 2 : 1), &a, sizeof(a), (unsigned int)((s->n_chains + 255) / 256), lds_split, stream);
        }
        if (e != hipSuccess && e != hipErrorNotFound) {
            (void)hipGetLastError(); /* a runtime that refuses the launch (e.g. the dynamic LDS size): the one-wave skeleton */
            e = hipErrorNotFound;
        }
        if (e == hipErrorNotFound) {
            const size_t lds = mm_tile_lds_bytes_rt(sizeof(T), s->dim);
            e = mm_rtc_launch_run(s->user, mh ? 0 : 1, std::is_same<T, float>::value ? 0 : 1, &a, sizeof(a), grid, s->block, lds, stream);
        }
        break;
    }
    case MM_LAUNCH_WIDE: {
        auto q = shared_args<mm_wide_args<T>>(a);
        q.P = P;
        q.kind = s->kind;
        q.dim = s->dim;
        q.eps = (T)s->scale;
        q.n_leapfrog = s->n_leapfrog;
        if constexpr (std::is_same<T, float>::value)
            e = mm_launch_hmc_wide_f32(q, stream);
        else
            e = mm_launch_hmc_wide_f64(q, stream);
        break;
    }
    case MM_LAUNCH_GENERIC: {
        auto q = shared_args<mm_gen_args<T>>(a);
        q.P = P;
        q.kind = s->kind;
        q.dim = s->dim;
        q.sampler = mh ? 0 : 1;
        q.scale = (T)s->scale;
        q.n_leapfrog = s->n_leapfrog;
        q.scratch = (T *)s->d_gscratch;
        q.c_pad = s->c_pad;
        if constexpr (std::is_same<T, float>::value)
            e = mm_launch_run_generic_f32(q, stream);
        else
            e = mm_launch_run_generic_f64(q, stream);
        break;
    }
    case MM_LAUNCH_LG: {
        auto q = shared_args<std::conditional_t<std::is_same<T, double>::value, mm_hmc_lg_args, mm_hmc_lg32_args>>(a);
        q.mat = (const T *)s->d_mat;
        q.eps = s->scale;
        q.n_leapfrog = s->n_leapfrog;
        if constexpr (std::is_same<T, double>::value)
            e = mm_launch_hmc_lg(s->dim, q, stream);
        else
            e = mm_launch_hmc_lg32(s->dim, q, stream);
        break;
    }
    case MM_LAUNCH_METRIC:
    case MM_LAUNCH_DENSE_METRIC: {
        /* the one-wave-per-SIMD skeleton around the target's functor with the metric, from the handle's diagonal or dense unit:
         * the kind decides which argument block is filled, and for a dense metric adds the staged factor to the LDS */
        mm_run_metric_args<T> md;
        mm_run_dense_args<T> mL;
        void *m = &md;
        size_t m_bytes = sizeof(md), lds = mm_tile_lds_bytes_rt(sizeof(T), s->dim);
        if (!s->caps.dense) {
            md.a = a;
            md.metric = (const T *)s->d_metric;
        } else {
            if (s->block != 64) /* mm_tile_lds_bytes_rt is the size for one wave per workgroup, which is what a unit is launched with */
                return MMCMC_ERR_STATE;
            mL.a = a;
            mL.chol = (const T *)s->d_metric;
            m = &mL, m_bytes = sizeof(mL);
            /* the body's dynamic LDS to a multiple of 16, then the staged factor (mm_kernels.h: mm_run_dense_lds) */
            lds = (lds + 15) / 16 * 16 + mm_tri_len((size_t)s->dim) * sizeof(T);
        }
        e = mm_rtc_launch_run(s->caps.dense ? s->dense_unit : s->metric_unit, 1, std::is_same<T, float>::value ? 0 : 1, m, m_bytes, grid, s->block, lds, stream);
        break;
    }
    case MM_LAUNCH_SEGMENTED: /* sampler_run runs such a schedule as unscheduled launches: sched_run is never set for it */
        return MMCMC_ERR_STATE;
    }
    if (e != hipSuccess)
        return (int)e;
    s->iter += (uint64_t)n_discard + n_collect;
    return MMCMC_OK;
}

/* the schedule of a run as mm_sched_step<T> [n + 1] in the handle's device buffer; eps converted as launch_range converts
 * s->scale.  Entry n ({0, 0}) is read by PIPE = 2's transition past an odd run's end, which changes nothing (ln u = NaN). */
template <class T> int upload_schedule(Sampler *s, const double *eps, const int32_t *L, size_t n, hipStream_t stream)
{
    const size_t bytes = (n + 1) * sizeof(mm_sched_step<T>);
    if (s->sched_pending) {
        MM_HIP(hipEventSynchronize(s->ev_sched)); /* the last scheduled run has read both buffers */
        s->sched_pending = false;
    }
    if (bytes > s->sched_cap) {
        if (s->d_sched)
            (void)hipFree(s->d_sched);
        s->d_sched = nullptr;
        s->sched_cap = 0;
        MM_HIP(hipMalloc(&s->d_sched, bytes));
        s->sched_cap = bytes;
    }
    if (!s->ev_sched)
        MM_HIP(hipEventCreateWithFlags(&s->ev_sched, hipEventDisableTiming));
    s->h_sched.assign(bytes, 0);
    mm_sched_step<T> *h = reinterpret_cast<mm_sched_step<T> *>(s->h_sched.data());
    for (size_t i = 0; i < n; ++i) {
        h[i].eps = (T)eps[i];
        h[i].n_leapfrog = L[i];
    }
    h[n].eps = T(0);
    h[n].n_leapfrog = 0;
    MM_HIP(hipMemcpyAsync(s->d_sched, s->h_sched.data(), bytes, hipMemcpyHostToDevice, stream));
    MM_HIP(hipEventRecord(s->ev_sched, stream)); /* recorded again after the run's launches */
    s->sched_pending = true;
    return MMCMC_OK;
}

/* n_total_rows / row0: the collected rows go to rows [row0, row0 + n_collect) of out [n_chains, n_total_rows, dim] (device
 * memory only when n_total_rows != n_collect): how run_progress fills one sample by several launches (mm_progress.hip).
 * sched_eps / sched_L (HMC, both or neither, checked by the caller): transition k of the run uses (sched_eps[k], sched_L[k])
 * -- read per transition by the scheduled kernels, else one launch per maximal run of equal pairs; the handle's own
 * step size and leapfrog count are what they were afterwards. */
int sampler_run(Sampler *s, size_t n_collect, size_t n_discard, void *out, int out_is_device,
                uint64_t *accept_counts, void *stream_v, size_t n_total_rows, size_t row0, const double *sched_eps,
                const int32_t *sched_L)
{
    if (!s)
        return MMCMC_ERR_INVALID_ARG;
    if (n_collect + n_discard == 0)
        return MMCMC_OK;
    if (n_total_rows == 0)
        n_total_rows = n_collect;
    if (row0 + n_collect > n_total_rows || ((n_total_rows != n_collect || row0 != 0) && out && !out_is_device))
        return MMCMC_ERR_INVALID_ARG;
    if ((uint64_t)n_total_rows * (uint64_t)s->dim >= (1ull << 30) || s->iter + n_collect + n_discard >= (1ull << 32))
        return MMCMC_ERR_SHAPE;
    DevGuard g(s->device);
    hipStream_t stream = stream_v ? (hipStream_t)stream_v : s->stream;
    /* a scheduled run: restores the handle's (eps, L) and leaves launch_range's scheduled mode however it returns */
    struct SchedScope {
        Sampler *s;
        double scale;
        int n_leapfrog;
        ~SchedScope()
        {
            s->scale = scale;
            s->n_leapfrog = n_leapfrog;
            s->sched_run = nullptr;
        }
    } sched_scope{s, s->scale, s->n_leapfrog};
    const bool sched = sched_eps != nullptr;
    if (sched && mm_launch_path(s->caps, s->variant, s->n_leapfrog, true) != MM_LAUNCH_SEGMENTED) {
        const int st = s->dtype == MMCMC_F32 ? upload_schedule<float>(s, sched_eps, sched_L, n_collect + n_discard, stream)
                                             : upload_schedule<double>(s, sched_eps, sched_L, n_collect + n_discard, stream);
        if (st != MMCMC_OK)
            return st;
        s->sched_run = s->d_sched;
        s->sched_iter0 = (uint32_t)s->iter; /* the RUN's first iteration: chunks index the schedule from here */
    }
    const size_t out_bytes = s->n_chains * n_collect * (size_t)s->dim * s->esize();
    void *d_out = nullptr;
    /* host output: the kernels write a device staging buffer the handle keeps (grown on demand, freed with the handle: a
     * hipMalloc + hipFree of the sample's size per call cost more than the kernel), mm_copy_to_host brings it over */
    bool staged = false;
    if (out && n_collect > 0) {
        if (out_is_device) {
            d_out = out;
        } else {
            if (out_bytes > s->stage_cap) {
                if (s->d_stage) {
                    MM_HIP(hipStreamSynchronize(stream));
                    (void)hipFree(s->d_stage);
                }
                s->d_stage = nullptr;
                s->stage_cap = 0;
                MM_HIP(hipMalloc(&s->d_stage, out_bytes));
                s->stage_cap = out_bytes;
            }
            d_out = s->d_stage;
            staged = true;
        }
    }
    /* per-chain accept counts only when asked for: otherwise neither the clearing fill nor the kernel's stores */
    s->want_accept = accept_counts != nullptr;
    if (s->want_accept)
        MM_HIP(hipMemsetAsync(s->d_accept, 0, s->n_chains * sizeof(unsigned long long), stream));

    /* split the run into launches of at most iters_per_launch transitions (0 = one launch) */
    uint64_t remaining_discard = n_discard, remaining_collect = n_collect, t0 = row0;
    const uint64_t cap = s->iters_per_launch ? s->iters_per_launch : (n_discard + n_collect);
    uint32_t launches = 0;
    const uint64_t n_run = (uint64_t)n_discard + n_collect;
    if (s->timing_enabled)
        MM_HIP(hipEventRecord(s->ev0, stream));
    while (remaining_discard + remaining_collect > 0) {
        uint64_t cap_k = cap;
        if (sched && !s->sched_run) {
            /* segmented fallback: this launch ends where the pair changes (one launch per transition at worst) */
            const uint64_t k = n_run - remaining_discard - remaining_collect;
            uint64_t len = 1;
            while (len < cap && k + len < n_run && sched_eps[k + len] == sched_eps[k] && sched_L[k + len] == sched_L[k])
                ++len;
            cap_k = len;
            s->scale = sched_eps[k];
            s->n_leapfrog = sched_L[k];
        }
        uint32_t nd = (uint32_t)std::min<uint64_t>(remaining_discard, cap_k);
        uint32_t nc = (uint32_t)std::min<uint64_t>(remaining_collect, cap_k - nd);
        int st;
        if (s->dtype == MMCMC_F32)
            st = launch_range<float>(s, s->kf, s->Pf, (float *)d_out, n_total_rows, nd, nc, (uint32_t)t0, stream);
        else
            st = launch_range<double>(s, s->kd, s->Pd, (double *)d_out, n_total_rows, nd, nc, (uint32_t)t0, stream);
        if (st != MMCMC_OK)
            return st;
        remaining_discard -= nd;
        remaining_collect -= nc;
        t0 += nc;
        ++launches;
    }
    if (s->sched_run) {
        MM_HIP(hipEventRecord(s->ev_sched, stream));
        s->sched_pending = true;
    }
    if (s->timing_enabled)
        MM_HIP(hipEventRecord(s->ev1, stream));
    s->timed = s->timing_enabled;
    s->timing.n_launches = launches;
    s->timing.out_bytes = d_out ? out_bytes : 0;
    s->timing.state_bytes = (uint64_t)launches * 2ull * s->n_chains * s->dim * s->esize();
    s->timing.kernel_ms = -1.0f;

    if (staged)
        MM_HIP(mm_copy_to_host(out, d_out, out_bytes, s->device, stream));
    if (accept_counts) {
        static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "u64");
        MM_HIP(hipMemcpyAsync(accept_counts, s->d_accept, s->n_chains * sizeof(uint64_t), hipMemcpyDeviceToHost,
                              stream));
        MM_HIP(hipStreamSynchronize(stream));
    }
    return MMCMC_OK;
}

int sampler_state(Sampler *s, void *out)
{
    if (!s || !out)
        return MMCMC_ERR_INVALID_ARG;
    DevGuard g(s->device);
    MM_HIP(hipStreamSynchronize(s->stream));
    MM_HIP(hipDeviceSynchronize());
    MM_HIP(hipMemcpy(out, s->d_state, s->n_chains * (size_t)s->dim * s->esize(), hipMemcpyDeviceToHost));
    return MMCMC_OK;
}

/* positions [n_chains, dim] of the handle's dtype from host memory (is_device = 0: copied before the call returns) or from
 * device memory on the handle's device, ordered on `stream` (NULL: the handle's own) like a run.  Every kernel variant
 * derives log-density and gradient from the state at launch: nothing else to invalidate. */
int sampler_set_state(Sampler *s, const void *positions, int is_device, void *stream)
{
    if (!s || !positions)
        return MMCMC_ERR_INVALID_ARG;
    DevGuard g(s->device);
    if (is_device) {
        hipPointerAttribute_t attr{};
        if (hipPointerGetAttributes(&attr, positions) != hipSuccess) {
            (void)hipGetLastError();
            return MMCMC_ERR_INVALID_ARG;
        }
        if ((attr.type != hipMemoryTypeDevice && !attr.isManaged) || attr.device != s->device)
            return MMCMC_ERR_INVALID_ARG;
    }
    hipStream_t st = stream ? (hipStream_t)stream : s->stream;
    MM_HIP(hipMemcpyAsync(s->d_state, positions, s->n_chains * (size_t)s->dim * s->esize(),
                          is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    if (!is_device)
        MM_HIP(hipStreamSynchronize(st)); /* the caller's host buffer is free again on return */
    return MMCMC_OK;
}

/* what keys the handle's future noise besides its positions: (seed, chain offset, iteration) */
int sampler_stream_position(const Sampler *s, uint64_t *seed, uint64_t *chain_offset, uint64_t *iteration)
{
    if (seed)
        *seed = s->seed;
    if (chain_offset)
        *chain_offset = s->chain_offset;
    if (iteration)
        *iteration = s->iter;
    return MMCMC_OK;
}

/* the next transition's iteration index; run() refuses to pass 2^32, so a counter there could never run again.  A run
 * already enqueued took its first iteration as a kernel argument: nothing on the device to order behind */
int sampler_set_iteration(Sampler *s, uint64_t iteration)
{
    if (iteration >= (1ull << 32))
        return MMCMC_ERR_INVALID_ARG;
    s->iter = iteration;
    return MMCMC_OK;
}

int sampler_sync(Sampler *s)
{
    if (!s)
        return MMCMC_ERR_INVALID_ARG;
    DevGuard g(s->device);
    if (s->timed)
        MM_HIP(hipEventSynchronize(s->ev1));
    MM_HIP(hipStreamSynchronize(s->stream));
    return MMCMC_OK;
}

int sampler_timing(Sampler *s, mmcmc_timing *t)
{
    if (!s || !t)
        return MMCMC_ERR_INVALID_ARG;
    if (!s->timed)
        return MMCMC_ERR_STATE; /* no timed run yet */
    DevGuard g(s->device);
    MM_HIP(hipEventSynchronize(s->ev1));
    float ms = 0.f;
    MM_HIP(hipEventElapsedTime(&ms, s->ev0, s->ev1));
    s->timing.kernel_ms = ms;
    *t = s->timing;
    return MMCMC_OK;
}

/* The metric unit's HMC kernel is checked once per (unit, dtype) and process before a handle relies on it, on the handle's own
 * parameter block (so a kind that carries data is checked on its data): up to 96 chains, 5 + 5 transitions with L = 3 from a
 * fixed start, (a) with a general metric twice -- the same bits --, (b) with a metric of all ones against the handle's
 * ordinary one-chain-per-lane kernel, which a ones-metric must reproduce bit for bit (mmcmc.h).  The handle's fields are
 * borrowed for the launches and put back.  Only real verdicts are cached.
 * dense: the dense-metric unit, checked the same way -- a general factor (large off-diagonal entries) twice, an identity
 * factor against the ordinary kernel. */
template <class T>
bool metric_unit_verified(Sampler *s, const mm_user_target *unit, const mm_tparams<T> &P, const mm_kernel_entry<T> *k, bool dense)
{
    static std::mutex mu;
    static std::map<std::pair<const void *, int>, bool> verdict;
    const std::pair<const void *, int> key{(const void *)unit, s->dtype};
    {
        std::lock_guard<std::mutex> l(mu);
        auto it = verdict.find(key);
        if (it != verdict.end())
            return it->second;
    }
    const size_t n = std::min<size_t>(96, s->n_chains), dim = (size_t)s->dim, nc = 5, nd = 5;
    const size_t n_met = dense ? mm_tri_len(dim) : dim;
    /* the probe inputs of mm_metric_host.h as the images a setter would upload; `ones` = no metric in either form */
    const std::vector<double> start = mm_probe_start(n, dim);
    const std::vector<T> x0(start.begin(), start.end());
    std::vector<T> ones(n_met, dense ? T(0) : T(1)), general, li;
    for (size_t i = 0; dense && i < dim; ++i)
        ones[mm_tri_len(i) + i] = T(1);
    if (dense ? !mm_dense_prepare<T>(mm_probe_chol(dim).data(), dim, general, li) : !mm_diag_prepare<T>(mm_probe_scale(dim).data(), dim, false, general))
        return false;
    /* the handle's fields the launches read, borrowed and put back */
    struct Borrow {
        Sampler *s;
        void *d_state, *d_metric;
        size_t n_chains;
        double scale;
        int n_leapfrog, variant, met_kind;
        uint64_t seed, chain_offset, iter;
        bool want_accept;
        const mm_user_target *unit, *dense_unit;
        const void *sched_run;
        ~Borrow()
        {
            s->d_state = d_state, s->d_metric = d_metric, s->n_chains = n_chains, s->scale = scale, s->n_leapfrog = n_leapfrog;
            s->variant = variant, s->seed = seed, s->chain_offset = chain_offset, s->iter = iter, s->want_accept = want_accept;
            s->met.kind = met_kind, s->metric_unit = unit, s->dense_unit = dense_unit, s->sched_run = sched_run;
            sync_metric_caps(s);
        }
    } borrow{s, s->d_state, s->d_metric, s->n_chains, s->scale, s->n_leapfrog, s->variant, s->met.kind, s->seed, s->chain_offset, s->iter,
             s->want_accept, s->metric_unit, s->dense_unit, s->sched_run};
    struct Dev {
        T *x = nullptr, *out = nullptr, *met = nullptr;
        ~Dev()
        {
            (void)hipFree(x);
            (void)hipFree(out);
            (void)hipFree(met);
        }
    } d;
    if (hipMalloc((void **)&d.x, n * dim * sizeof(T)) != hipSuccess || hipMalloc((void **)&d.out, n * nc * dim * sizeof(T)) != hipSuccess ||
        hipMalloc((void **)&d.met, n_met * sizeof(T)) != hipSuccess)
        return false;
    s->d_state = d.x;
    s->d_metric = d.met;
    s->n_chains = n;
    s->seed = 0x5eedull;
    s->chain_offset = 0;
    s->scale = 0.01; /* modest fixed scales, as builtin_unit_verified: the check is about the kernels */
    s->n_leapfrog = 3;
    s->want_accept = false;
    s->sched_run = nullptr;
    (dense ? s->dense_unit : s->metric_unit) = unit;
    /* the one-chain-per-lane kernel the handle has without a metric: its unit, its fixed-dimension kernel, or run-time D */
    const int plain = s->caps.unit != MM_UNIT_NONE ? MM_VAR_UNIT : s->caps.fixed ? (s->dim > 16 ? MM_VAR_PLAIN : MM_VAR_PAIRED) : MM_VAR_GENERIC;
    /* metric == nullptr: the ordinary kernel */
    auto one = [&](const std::vector<T> *metric, std::vector<T> &got) -> bool {
        got.assign(n * nc * dim, T(0));
        s->iter = 0;
        s->met.kind = !metric ? MM_METRIC_NONE : dense ? MM_METRIC_DENSE : MM_METRIC_DIAG;
        sync_metric_caps(s);
        s->variant = metric ? MM_VAR_UNIT : plain;
        return (!metric || hipMemcpy(d.met, metric->data(), n_met * sizeof(T), hipMemcpyHostToDevice) == hipSuccess) &&
               hipMemcpy(d.x, x0.data(), n * dim * sizeof(T), hipMemcpyHostToDevice) == hipSuccess &&
               launch_range<T>(s, k, P, d.out, nc, (uint32_t)nd, (uint32_t)nc, 0, s->stream) == MMCMC_OK &&
               hipStreamSynchronize(s->stream) == hipSuccess &&
               hipMemcpy(got.data(), d.out, got.size() * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess;
    };
    std::vector<T> g1, g2, u1, p0;
    if (!one(&general, g1) || !one(&general, g2) || !one(&ones, u1) || !one(nullptr, p0))
        return false; /* an allocation or launch error: no verdict, the next set_metric tries again */
    auto same = [](const std::vector<T> &a, const std::vector<T> &b) { return std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0; };
    const bool ok = same(g1, g2) && same(u1, p0);
    std::lock_guard<std::mutex> l(mu);
    verdict[key] = ok;
    return ok;
}

/* mmcmc_hmc_set_metric (dense = false: values = the scales [dim]) and mmcmc_hmc_set_metric_dense (values = L row-major
 * [dim, dim]): every check before any change, nothing changed on any refusal */
template <class T> int sampler_set_metric_t(Sampler *s, bool dense, const double *values)
{
    const size_t dim = (size_t)s->dim;
    /* HMC's kernels never read r_i = 1 / s_i, so the diagonal image is s alone (mm_diag_prepare); li is NUTS's, and forming it
     * here keeps the dense checks the same for both samplers */
    std::vector<T> image, li;
    if (dense ? !mm_dense_prepare<T>(values, dim, image, li) : !mm_diag_prepare<T>(values, dim, false, image))
        return MMCMC_ERR_INVALID_ARG;
    /* the dense unit's launch sizes its LDS for one wave per workgroup */
    if (mm_metric_status(s->caps) != MMCMC_OK || (dense && s->block != 64))
        return MMCMC_ERR_UNSUPPORTED;
    DevGuard g(s->device);
    const mm_user_target *&kept = dense ? s->dense_unit : s->metric_unit;
    const mm_user_target *unit = kept ? kept : mm_rtc_metric_unit(s->kind, s->dim, dense);
    if (!unit) /* no run-time compiler, a kind without a gradient functor (a model's handle carries the model's kind), or the unit does not build */
        return MMCMC_ERR_UNSUPPORTED;
    MM_HIP(hipDeviceSynchronize()); /* behind every queued run: a metric applies from the next transition on */
    bool verified;
    if constexpr (std::is_same<T, float>::value)
        verified = metric_unit_verified<float>(s, unit, s->Pf, s->kf, dense);
    else
        verified = metric_unit_verified<double>(s, unit, s->Pd, s->kd, dense);
    if (!verified)
        return MMCMC_ERR_UNSUPPORTED;
    if (!s->d_metric) /* room for either kind: a dense metric's packed factor */
        MM_HIP(hipMalloc(&s->d_metric, mm_tri_len(dim) * sizeof(T)));
    MM_HIP(hipMemcpy(s->d_metric, image.data(), image.size() * sizeof(T), hipMemcpyHostToDevice));
    kept = unit;
    if (dense)
        s->met.commit_dense(values, dim, s->variant);
    else
        s->met.commit_diag(values, dim, s->variant);
    sync_metric_caps(s);
    return MMCMC_OK;
}
int sampler_set_metric(Sampler *s, bool dense, const double *values)
{
    if (!values) { /* the identity, through either entry point: back to the variant the handle had */
        s->met.clear(s->variant);
        sync_metric_caps(s);
        return MMCMC_OK;
    }
    if (dense && s->dim < 1) /* nothing to read */
        return MMCMC_ERR_INVALID_ARG;
    return s->dtype == MMCMC_F32 ? sampler_set_metric_t<float>(s, dense, values) : sampler_set_metric_t<double>(s, dense, values);
}

template <class T>
int logp_grad_batch_t(const mmcmc_target_desc *target, const void *x, size_t n, void *logp, void *grad)
{
    const mm_user_target *user = target->kind >= MM_USER_KIND_BASE ? mm_rtc_find(target->kind) : nullptr;
    const mm_kernel_entry<T> *k = user ? nullptr : find_kernel<T>(target->kind, target->dim);
    if (!k && !user && !mm_generic_kind_ok(target->kind))
        return MMCMC_ERR_UNSUPPORTED;
    mm_tparams<T> P;
    T *d_mat = nullptr;
    int st = make_params<T>(target, &P, &d_mat);
    if (st != MMCMC_OK)
        return st;
    size_t d = (size_t)target->dim;
    T *dx = nullptr, *dl = nullptr, *dg = nullptr, *dscr = nullptr;
    int rc = MMCMC_OK;
    hipError_t e;
    do {
        if ((e = hipMalloc((void **)&dx, n * d * sizeof(T))) != hipSuccess)
            break;
        if ((e = hipMalloc((void **)&dl, n * sizeof(T))) != hipSuccess)
            break;
        if (grad && (e = hipMalloc((void **)&dg, n * d * sizeof(T))) != hipSuccess)
            break;
        if ((e = hipMemcpy(dx, x, n * d * sizeof(T), hipMemcpyHostToDevice)) != hipSuccess)
            break;
        if (user) {
            struct {
                mm_tparams<T> P;
                const T *x;
                T *logp, *grad;
                unsigned long long n;
            } ua{P, dx, dl, dg, (unsigned long long)n};
            if ((e = mm_rtc_launch_logp_grad(user, std::is_same<T, float>::value ? 0 : 1, &ua, sizeof(ua), n, nullptr)) != hipSuccess)
                break;
        } else if (k) {
            if ((e = k->logp_grad(P, dx, dl, dg, (unsigned long long)n, nullptr)) != hipSuccess)
                break;
        } else {
            /* run-time dimension: position and gradient of row i in a lane-interleaved scratch store */
            const unsigned long long n_pad = (n + 63) / 64 * 64;
            if ((e = hipMalloc((void **)&dscr, 2 * d * n_pad * sizeof(T))) != hipSuccess)
                break;
            if constexpr (std::is_same<T, float>::value)
                e = mm_launch_logp_grad_generic_f32(P, target->kind, target->dim, dx, dl, dg, dscr, n, n_pad, nullptr);
            else
                e = mm_launch_logp_grad_generic_f64(P, target->kind, target->dim, dx, dl, dg, dscr, n, n_pad, nullptr);
            if (e != hipSuccess)
                break;
        }
        if ((e = hipDeviceSynchronize()) != hipSuccess)
            break;
        if ((e = hipMemcpy(logp, dl, n * sizeof(T), hipMemcpyDeviceToHost)) != hipSuccess)
            break;
        if (grad && (e = hipMemcpy(grad, dg, n * d * sizeof(T), hipMemcpyDeviceToHost)) != hipSuccess)
            break;
    } while (0);
    if (e != hipSuccess)
        rc = (int)e;
    (void)hipFree(dx);
    (void)hipFree(dl);
    if (dg)
        (void)hipFree(dg);
    if (dscr)
        (void)hipFree(dscr);
    if (d_mat)
        (void)hipFree(d_mat);
    return rc;
}

template <class T>
int draw_noise_t(uint64_t seed, uint64_t chain_offset, uint32_t iteration, size_t n, int dim, void *z, void *u, int mh = 0)
{
    int nn = 0;
    const mm_noise_entry<T> *t = noise_table<T>(&nn);
    const mm_noise_entry<T> *k = nullptr;
    /* mh: the MH sampler's paired stream (f32, dim <= 2: mm_rng.h) through the run-time-dimension kernel; the same noise as
     * mmcmc_draw_noise's everywhere else */
    const bool paired = mh && std::is_same<T, float>::value && dim <= 2;
    for (int i = 0; i < nn && !paired; ++i)
        if (t[i].dim == dim)
            k = &t[i];
    if (!k && dim <= 0)
        return MMCMC_ERR_INVALID_ARG;
    T *dz = nullptr, *du = nullptr;
    hipError_t e;
    do {
        if ((e = hipMalloc((void **)&dz, n * (size_t)dim * sizeof(T))) != hipSuccess)
            break;
        if ((e = hipMalloc((void **)&du, n * sizeof(T))) != hipSuccess)
            break;
        if (k)
            e = k->noise(seed, chain_offset, iteration, (unsigned long long)n, dz, du, nullptr);
        else if constexpr (std::is_same<T, float>::value)
            e = mm_launch_noise_generic_f32(seed, chain_offset, iteration, dim, (unsigned long long)n, dz, du, nullptr, paired ? 1 : 0);
        else
            e = mm_launch_noise_generic_f64(seed, chain_offset, iteration, dim, (unsigned long long)n, dz, du, nullptr);
        if (e != hipSuccess)
            break;
        if ((e = hipDeviceSynchronize()) != hipSuccess)
            break;
        if ((e = hipMemcpy(z, dz, n * (size_t)dim * sizeof(T), hipMemcpyDeviceToHost)) != hipSuccess)
            break;
        if ((e = hipMemcpy(u, du, n * sizeof(T), hipMemcpyDeviceToHost)) != hipSuccess)
            break;
    } while (0);
    (void)hipFree(dz);
    (void)hipFree(du);
    return e == hipSuccess ? MMCMC_OK : (int)e;
}

} // namespace

/* ------------------------------------------------------------------ C ABI */

struct mmcmc_mh {
    Sampler *s;
};
struct mmcmc_hmc {
    Sampler *s;
};

extern "C" {

int mmcmc_version(void) { return MMCMC_VERSION; }

const char *mmcmc_status_string(int status)
{
    switch (status) {
    case MMCMC_OK:
        return "ok";
    case MMCMC_ERR_INVALID_ARG:
        return "invalid argument";
    case MMCMC_ERR_UNSUPPORTED:
        return "unsupported target kind / dimension / element type";
    case MMCMC_ERR_SHAPE:
        return "shape error";
    case MMCMC_ERR_NO_DEVICE:
        return "no HIP device (the engine has no CPU fallback)";
    case MMCMC_ERR_STATE:
        return "handle in the wrong state";
    case MMCMC_ERR_GROUP_BROKEN:
        return "device group broken: a run failed after some shards had advanced";
    default:
        return status > 0 ? hipGetErrorString((hipError_t)status) : "unknown status";
    }
}

int mmcmc_device_pci_bus_id(int device, char *buf, size_t len)
{
    if (!buf || len < 16)
        return MMCMC_ERR_INVALID_ARG;
    buf[0] = 0;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return MMCMC_ERR_NO_DEVICE;
    if (device < 0 || device >= n)
        return MMCMC_ERR_INVALID_ARG;
    const hipError_t e = hipDeviceGetPCIBusId(buf, (int)len, device);
    return e == hipSuccess ? MMCMC_OK : (int)e;
}

int mmcmc_device_count(int *count)
{
    if (!count)
        return MMCMC_ERR_INVALID_ARG;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        *count = 0;
        return MMCMC_ERR_NO_DEVICE;
    }
    *count = n;
    return MMCMC_OK;
}

int mmcmc_init_with_seed(size_t n, size_t d, uint64_t seed, double *out)
{
    if (!out && n * d > 0)
        return MMCMC_ERR_INVALID_ARG;
    mm_host::SmallRng rng(seed);
    for (size_t i = 0; i < n * d; ++i)
        out[i] = rng.standard_normal();
    return MMCMC_OK;
}

/* ---- MH ---- */
int mmcmc_mh_create(mmcmc_mh **out, const mmcmc_target_desc *target, const mmcmc_proposal_desc *proposal,
                    const void *init, size_t n_chains, int dtype, int device)
{
    if (!out || !proposal)
        return MMCMC_ERR_INVALID_ARG;
    *out = nullptr;
    Sampler *s = nullptr;
    int st;
    if (proposal->kind >= MMCMC_USER_PROPOSAL_BASE) {
        /* a proposal compiled from source (mmcmc_proposal_register_source): the target + proposal model stands in for the
         * target; it was compiled for exactly one target kind and dimension */
        const mm_user_target *model = mm_rtc_find(proposal->kind);
        if (!model || !mm_rtc_is_model(model) || !target)
            return MMCMC_ERR_UNSUPPORTED;
        if (mm_rtc_base_kind(model) != target->kind)
            return MMCMC_ERR_UNSUPPORTED;
        if (mm_rtc_dim(model) != target->dim)
            return MMCMC_ERR_SHAPE;
        if (target->kind < MM_USER_KIND_BASE) { /* the built-in target's own description must be valid */
            st = validate_target(target);
            if (st != MMCMC_OK)
                return st;
        }
        mmcmc_target_desc as_model = *target;
        as_model.kind = proposal->kind;
        g_allow_model = true;
        st = sampler_create(&s, MM_SAMPLER_MH, &as_model, proposal->std, 0, init, n_chains, dtype, device);
        g_allow_model = false;
    } else if (proposal->kind != MMCMC_PROPOSAL_ISOTROPIC_GAUSSIAN) {
        return MMCMC_ERR_UNSUPPORTED;
    } else {
        st = sampler_create(&s, MM_SAMPLER_MH, target, proposal->std, 0, init, n_chains, dtype, device);
    }
    if (st != MMCMC_OK)
        return st;
    mmcmc_mh *h = new (std::nothrow) mmcmc_mh{s};
    if (!h) {
        sampler_destroy(s);
        return (int)hipErrorOutOfMemory;
    }
    *out = h;
    return MMCMC_OK;
}
int mmcmc_mh_seed(mmcmc_mh *h, uint64_t seed)
{
    if (!h)
        return MMCMC_ERR_INVALID_ARG;
    h->s->seed = seed;
    return MMCMC_OK;
}
int mmcmc_mh_set_chain_offset(mmcmc_mh *h, uint64_t off)
{
    if (!h)
        return MMCMC_ERR_INVALID_ARG;
    h->s->chain_offset = off;
    return MMCMC_OK;
}
/* which variants a handle takes: mm_variant_status (mm_path.h), the MH and HMC ranges included */
static int sampler_set_variant(Sampler *s, int variant)
{
    const int st = mm_variant_status(s->caps, variant);
    if (st == MMCMC_OK)
        s->variant = variant;
    return st;
}
int mmcmc_mh_set_kernel_variant(mmcmc_mh *h, int variant)
{
    return h ? sampler_set_variant(h->s, variant) : MMCMC_ERR_INVALID_ARG;
}
int mmcmc_hmc_set_kernel_variant(mmcmc_hmc *h, int variant)
{
    return h ? sampler_set_variant(h->s, variant) : MMCMC_ERR_INVALID_ARG;
}
int mmcmc_hmc_kernel_variant(mmcmc_hmc *h) { return h ? h->s->variant : MMCMC_ERR_INVALID_ARG; }
int mmcmc_mh_enable_timing(mmcmc_mh *h, int on)
{
    if (!h)
        return MMCMC_ERR_INVALID_ARG;
    h->s->timing_enabled = on != 0;
    return MMCMC_OK;
}
int mmcmc_hmc_enable_timing(mmcmc_hmc *h, int on)
{
    if (!h)
        return MMCMC_ERR_INVALID_ARG;
    h->s->timing_enabled = on != 0;
    return MMCMC_OK;
}
int mmcmc_mh_set_iters_per_launch(mmcmc_mh *h, uint32_t iters)
{
    if (!h)
        return MMCMC_ERR_INVALID_ARG;
    h->s->iters_per_launch = iters;
    return MMCMC_OK;
}
int mmcmc_mh_run(mmcmc_mh *h, size_t n_collect, size_t n_discard, void *out, int out_is_device,
                 uint64_t *accept_counts, void *stream)
{
    return h ? sampler_run(h->s, n_collect, n_discard, out, out_is_device, accept_counts, stream)
             : MMCMC_ERR_INVALID_ARG;
}
int mmcmc_mh_run_rows(mmcmc_mh *h, size_t n_rows, size_t n_discard, void *out_device, size_t n_total_rows, size_t row0,
                      void *stream)
{
    return h ? sampler_run(h->s, n_rows, n_discard, out_device, 1, nullptr, stream, n_total_rows, row0) : MMCMC_ERR_INVALID_ARG;
}
static int sampler_shape(const Sampler *s, size_t *n_chains, int *dim, int *dtype, int *device)
{
    if (n_chains)
        *n_chains = s->n_chains;
    if (dim)
        *dim = s->dim;
    if (dtype)
        *dtype = s->dtype;
    if (device)
        *device = s->device;
    return MMCMC_OK;
}
int mmcmc_mh_shape(mmcmc_mh *h, size_t *n_chains, int *dim, int *dtype, int *device)
{
    return h ? sampler_shape(h->s, n_chains, dim, dtype, device) : MMCMC_ERR_INVALID_ARG;
}
int mmcmc_mh_state(mmcmc_mh *h, void *out) { return h ? sampler_state(h->s, out) : MMCMC_ERR_INVALID_ARG; }
int mmcmc_mh_sync(mmcmc_mh *h) { return h ? sampler_sync(h->s) : MMCMC_ERR_INVALID_ARG; }
int mmcmc_mh_timing(mmcmc_mh *h, mmcmc_timing *t) { return h ? sampler_timing(h->s, t) : MMCMC_ERR_INVALID_ARG; }
/* the reference's public fields (metropolis_hastings.rs:101-109: pub proposal, pub current_state) -- from the next
 * transition on; seed, chain offset and iteration untouched */
int mmcmc_mh_set_proposal_std(mmcmc_mh *h, double std)
{
    if (!h || !(std > 0.0) || !std::isfinite(std)) /* mmcmc_mh_create's check */
        return MMCMC_ERR_INVALID_ARG;
    h->s->scale = std;
    return MMCMC_OK;
}
int mmcmc_mh_params(mmcmc_mh *h, double *std)
{
    if (!h)
        return MMCMC_ERR_INVALID_ARG;
    if (std)
        *std = h->s->scale;
    return MMCMC_OK;
}
int mmcmc_mh_set_state(mmcmc_mh *h, const void *x, int is_device, void *stream)
{
    return h ? sampler_set_state(h->s, x, is_device, stream) : MMCMC_ERR_INVALID_ARG;
}
int mmcmc_mh_stream_position(mmcmc_mh *h, uint64_t *seed, uint64_t *chain_offset, uint64_t *iteration)
{
    return h ? sampler_stream_position(h->s, seed, chain_offset, iteration) : MMCMC_ERR_INVALID_ARG;
}
int mmcmc_mh_set_iteration(mmcmc_mh *h, uint64_t iteration)
{
    return h ? sampler_set_iteration(h->s, iteration) : MMCMC_ERR_INVALID_ARG;
}
int mmcmc_mh_destroy(mmcmc_mh *h)
{
    if (!h)
        return MMCMC_ERR_INVALID_ARG;
    int st = sampler_destroy(h->s);
    delete h;
    return st;
}

/* ---- HMC ---- */
int mmcmc_hmc_create(mmcmc_hmc **out, const mmcmc_target_desc *target, const void *init, size_t n_chains,
                     double step_size, int n_leapfrog, int dtype, int device)
{
    if (!out)
        return MMCMC_ERR_INVALID_ARG;
    *out = nullptr;
    Sampler *s = nullptr;
    int st = sampler_create(&s, MM_SAMPLER_HMC, target, step_size, n_leapfrog, init, n_chains, dtype, device);
    if (st != MMCMC_OK)
        return st;
    mmcmc_hmc *h = new (std::nothrow) mmcmc_hmc{s};
    if (!h) {
        sampler_destroy(s);
        return (int)hipErrorOutOfMemory;
    }
    *out = h;
    return MMCMC_OK;
}
int mmcmc_hmc_seed(mmcmc_hmc *h, uint64_t seed)
{
    if (!h)
        return MMCMC_ERR_INVALID_ARG;
    h->s->seed = seed;
    return MMCMC_OK;
}
int mmcmc_hmc_set_chain_offset(mmcmc_hmc *h, uint64_t off)
{
    if (!h)
        return MMCMC_ERR_INVALID_ARG;
    h->s->chain_offset = off;
    return MMCMC_OK;
}
int mmcmc_hmc_set_iters_per_launch(mmcmc_hmc *h, uint32_t iters)
{
    if (!h)
        return MMCMC_ERR_INVALID_ARG;
    h->s->iters_per_launch = iters;
    return MMCMC_OK;
}
int mmcmc_hmc_run(mmcmc_hmc *h, size_t n_collect, size_t n_discard, void *out, int out_is_device,
                  uint64_t *accept_counts, void *stream)
{
    return h ? sampler_run(h->s, n_collect, n_discard, out, out_is_device, accept_counts, stream)
             : MMCMC_ERR_INVALID_ARG;
}
int mmcmc_hmc_run_rows(mmcmc_hmc *h, size_t n_rows, size_t n_discard, void *out_device, size_t n_total_rows, size_t row0,
                       void *stream)
{
    return h ? sampler_run(h->s, n_rows, n_discard, out_device, 1, nullptr, stream, n_total_rows, row0) : MMCMC_ERR_INVALID_ARG;
}
int mmcmc_hmc_shape(mmcmc_hmc *h, size_t *n_chains, int *dim, int *dtype, int *device)
{
    return h ? sampler_shape(h->s, n_chains, dim, dtype, device) : MMCMC_ERR_INVALID_ARG;
}
int mmcmc_hmc_step(mmcmc_hmc *h, void *stream)
{
    return h ? sampler_run(h->s, 0, 1, nullptr, 1, nullptr, stream) : MMCMC_ERR_INVALID_ARG;
}
int mmcmc_hmc_state(mmcmc_hmc *h, void *out) { return h ? sampler_state(h->s, out) : MMCMC_ERR_INVALID_ARG; }
/* the reference's public fields (hmc.rs:41-49): step_size, n_leapfrog, positions -- from the next transition on */
int mmcmc_hmc_set_step_size(mmcmc_hmc *h, double step_size)
{
    if (!h || !(step_size > 0.0) || !std::isfinite(step_size)) /* mmcmc_hmc_create's check */
        return MMCMC_ERR_INVALID_ARG;
    h->s->scale = step_size;
    return MMCMC_OK;
}
int mmcmc_hmc_set_n_leapfrog(mmcmc_hmc *h, int n_leapfrog)
{
    if (!h || n_leapfrog < 0)
        return MMCMC_ERR_INVALID_ARG;
    h->s->n_leapfrog = n_leapfrog;
    return MMCMC_OK;
}
int mmcmc_hmc_params(mmcmc_hmc *h, double *step_size, int *n_leapfrog)
{
    if (!h)
        return MMCMC_ERR_INVALID_ARG;
    if (step_size)
        *step_size = h->s->scale;
    if (n_leapfrog)
        *n_leapfrog = h->s->n_leapfrog;
    return MMCMC_OK;
}
int mmcmc_hmc_set_metric(mmcmc_hmc *h, const double *scale) { return h ? sampler_set_metric(h->s, false, scale) : MMCMC_ERR_INVALID_ARG; }
int mmcmc_hmc_metric(mmcmc_hmc *h, double *scale_out)
{
    return h && scale_out ? h->s->met.report_scale(scale_out, (size_t)h->s->dim) : MMCMC_ERR_INVALID_ARG;
}
int mmcmc_hmc_set_metric_dense(mmcmc_hmc *h, const double *chol) { return h ? sampler_set_metric(h->s, true, chol) : MMCMC_ERR_INVALID_ARG; }
int mmcmc_hmc_metric_dense(mmcmc_hmc *h, double *chol_out) { return h && chol_out ? h->s->met.report_chol(chol_out) : MMCMC_ERR_INVALID_ARG; }
int mmcmc_hmc_set_state(mmcmc_hmc *h, const void *positions, int is_device, void *stream)
{
    return h ? sampler_set_state(h->s, positions, is_device, stream) : MMCMC_ERR_INVALID_ARG;
}
int mmcmc_hmc_stream_position(mmcmc_hmc *h, uint64_t *seed, uint64_t *chain_offset, uint64_t *iteration)
{
    return h ? sampler_stream_position(h->s, seed, chain_offset, iteration) : MMCMC_ERR_INVALID_ARG;
}
int mmcmc_hmc_set_iteration(mmcmc_hmc *h, uint64_t iteration)
{
    return h ? sampler_set_iteration(h->s, iteration) : MMCMC_ERR_INVALID_ARG;
}
int mmcmc_hmc_run_scheduled(mmcmc_hmc *h, size_t n_collect, size_t n_discard, const double *step_sizes,
                            const int32_t *n_leapfrogs, void *out, int out_is_device, uint64_t *accept_counts, void *stream)
{
    if (!h)
        return MMCMC_ERR_INVALID_ARG;
    const size_t n = n_collect + n_discard;
    if (n == 0)
        return MMCMC_OK;
    if (!step_sizes || !n_leapfrogs)
        return MMCMC_ERR_INVALID_ARG;
    for (size_t k = 0; k < n; ++k)
        if (!(step_sizes[k] > 0.0) || !std::isfinite(step_sizes[k]) || n_leapfrogs[k] < 0)
            return MMCMC_ERR_INVALID_ARG;
    return sampler_run(h->s, n_collect, n_discard, out, out_is_device, accept_counts, stream, 0, 0, step_sizes, n_leapfrogs);
}
int mmcmc_hmc_sync(mmcmc_hmc *h) { return h ? sampler_sync(h->s) : MMCMC_ERR_INVALID_ARG; }
int mmcmc_hmc_timing(mmcmc_hmc *h, mmcmc_timing *t) { return h ? sampler_timing(h->s, t) : MMCMC_ERR_INVALID_ARG; }
int mmcmc_hmc_destroy(mmcmc_hmc *h)
{
    if (!h)
        return MMCMC_ERR_INVALID_ARG;
    int st = sampler_destroy(h->s);
    delete h;
    return st;
}

/* ---- densities / noise (parity tests) ---- */
int mmcmc_logp_grad_batch(const mmcmc_target_desc *target, int dtype, const void *x, size_t n, void *logp,
                          void *grad, int device)
{
    if (!x || !logp || n == 0 || (dtype != MMCMC_F32 && dtype != MMCMC_F64))
        return MMCMC_ERR_INVALID_ARG;
    int st = validate_target(target);
    if (st != MMCMC_OK)
        return st;
    st = mm_check_device(device);
    if (st != MMCMC_OK)
        return st;
    DevGuard g(device);
    return dtype == MMCMC_F32 ? logp_grad_batch_t<float>(target, x, n, logp, grad)
                              : logp_grad_batch_t<double>(target, x, n, logp, grad);
}

int mmcmc_draw_noise(uint64_t seed, uint64_t chain_offset, uint32_t iteration, size_t n_chains, int dim, int dtype,
                     void *z, void *u, int device)
{
    if (!z || !u || n_chains == 0 || dim <= 0 || (dtype != MMCMC_F32 && dtype != MMCMC_F64))
        return MMCMC_ERR_INVALID_ARG;
    int st = mm_check_device(device);
    if (st != MMCMC_OK)
        return st;
    DevGuard g(device);
    return dtype == MMCMC_F32 ? draw_noise_t<float>(seed, chain_offset, iteration, n_chains, dim, z, u)
                              : draw_noise_t<double>(seed, chain_offset, iteration, n_chains, dim, z, u);
}

int mmcmc_draw_noise_mh(uint64_t seed, uint64_t chain_offset, uint32_t iteration, size_t n_chains, int dim, int dtype,
                        void *z, void *u, int device)
{
    if (!z || !u || n_chains == 0 || dim <= 0 || (dtype != MMCMC_F32 && dtype != MMCMC_F64))
        return MMCMC_ERR_INVALID_ARG;
    int st = mm_check_device(device);
    if (st != MMCMC_OK)
        return st;
    DevGuard g(device);
    return dtype == MMCMC_F32 ? draw_noise_t<float>(seed, chain_offset, iteration, n_chains, dim, z, u, 1)
                              : draw_noise_t<double>(seed, chain_offset, iteration, n_chains, dim, z, u, 1);
}

} /* extern "C" */
