/*
 * mmcmc.hpp -- header-only C++17 facade over the C ABI (mmcmc.h), shaped like the reference crate's surface.
 *
 * The reference is Rust; with no Rust toolchain in this image the host side above the C ABI is C++ (this file) and
 * Python (mini_mcmc_amd/).  Names, argument meaning and error behaviour follow the crate:
 *     mini_mcmc::core::{init_det, init_with_seed}              core.rs:394-435
 *     mini_mcmc::distributions::{Gaussian2D, DiffableGaussian2D, IsotropicGaussian, Rosenbrock2D, RosenbrockND}
 *     mini_mcmc::metropolis_hastings::MetropolisHastings::{new, seed} + ChainRunner::run   (core.rs:176-186)
 *     mini_mcmc::hmc::HMC::{new, set_seed, run, step}          hmc.rs:87-158, 304-377
 *     mini_mcmc::nuts::NUTS::{new, set_seed, run}              nuts.rs:123-170, 347-353
 *     mini_mcmc::stats::{split_rhat_mean_ess, RunStats}        stats.rs:339-423
 * Samples come back as a flat row-major std::vector with shape [n_chains, n_collect, dim] (Array3 / Tensor<B,3>).
 * Rust's `Result<_, ShapeError>` / panics become the exception mmcmc::Error carrying the C status.
 */
#ifndef MMCMC_HPP
#define MMCMC_HPP

#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <memory>
#include <vector>

#include "mmcmc.h"

namespace mmcmc {

struct Error : std::runtime_error {
    int status;
    Error(int st, const std::string &where)
        : std::runtime_error(where + ": " + mmcmc_status_string(st) + " (" + std::to_string(st) + ")"), status(st)
    {
    }
};
inline void check(int st, const char *where)
{
    if (st != MMCMC_OK)
        throw Error(st, where);
}

template <class T> constexpr int dtype_of()
{
    static_assert(std::is_same<T, float>::value || std::is_same<T, double>::value, "f32 or f64");
    return std::is_same<T, float>::value ? MMCMC_F32 : MMCMC_F64;
}

/* core.rs:413-419 / :404-409 : row-major [n, d] */
template <class T> std::vector<T> init_with_seed(size_t n, size_t d, uint64_t seed)
{
    std::vector<double> tmp(n * d);
    check(mmcmc_init_with_seed(n, d, seed, tmp.data()), "mmcmc_init_with_seed");
    return std::vector<T>(tmp.begin(), tmp.end());
}
template <class T> std::vector<T> init_det(size_t n, size_t d) { return init_with_seed<T>(n, d, 42); }

/* what keys a handle's next transition besides its positions (include/mmcmc.h: chain state and stream position) */
struct StreamPosition {
    uint64_t seed = 0, chain_offset = 0, iteration = 0;
};

/* ---- distributions ---- */
struct Target {
    mmcmc_target_desc d{};
    std::vector<double> matrix;
    const mmcmc_target_desc *desc()
    {
        d.matrix = matrix.empty() ? nullptr : matrix.data();
        return &d;
    }
};
inline Target Gaussian2D(std::array<double, 2> mean, std::array<std::array<double, 2>, 2> cov, bool diffable = false)
{
    Target t;
    t.d.kind = diffable ? MMCMC_DIFFABLE_GAUSSIAN2D : MMCMC_GAUSSIAN2D;
    t.d.dim = 2;
    t.d.params[0] = mean[0];
    t.d.params[1] = mean[1];
    t.d.params[2] = cov[0][0];
    t.d.params[3] = cov[0][1];
    t.d.params[4] = cov[1][0];
    t.d.params[5] = cov[1][1];
    return t;
}
inline Target DiffableGaussian2D(std::array<double, 2> mean, std::array<std::array<double, 2>, 2> cov)
{
    return Gaussian2D(mean, cov, true);
}
inline Target Rosenbrock2D(double a, double b)
{
    Target t;
    t.d.kind = MMCMC_ROSENBROCK2D;
    t.d.dim = 2;
    t.d.params[0] = a;
    t.d.params[1] = b;
    return t;
}
inline Target RosenbrockND(int dim)
{
    Target t;
    t.d.kind = MMCMC_ROSENBROCK_ND;
    t.d.dim = dim;
    return t;
}
inline Target StandardNormal(int dim)
{
    Target t;
    t.d.kind = MMCMC_STANDARD_NORMAL;
    t.d.dim = dim;
    return t;
}
inline Target GaussianND(int dim, std::vector<double> precision)
{
    Target t;
    t.d.kind = MMCMC_GAUSSIAN_ND;
    t.d.dim = dim;
    t.matrix = std::move(precision);
    return t;
}
struct IsotropicGaussian {
    double std;
    explicit IsotropicGaussian(double s) : std(s) {}
    IsotropicGaussian set_seed(uint64_t) const { return *this; } /* the engine's stream is keyed by the sampler */
    Target as_target(int dim) const
    {
        Target t;
        t.d.kind = MMCMC_ISOTROPIC_GAUSSIAN;
        t.d.dim = dim;
        t.d.params[0] = std;
        return t;
    }
};

/* ---- stats ---- */
struct RunStats {
    mmcmc_run_stats s{};
};
inline std::pair<std::vector<float>, std::vector<float>> split_rhat_mean_ess(const std::vector<float> &sample,
                                                                              size_t chains, size_t n, size_t dim,
                                                                              int device = 0)
{
    std::vector<float> rhat(dim), ess(dim);
    check(mmcmc_split_rhat_mean_ess(sample.data(), 0, MMCMC_F32, chains, n, dim, rhat.data(), ess.data(), device,
                                    nullptr),
          "mmcmc_split_rhat_mean_ess");
    return {rhat, ess};
}

/* Rank-normalised diagnostics (Vehtari et al. 2021; mmcmc.h "rank-normalised diagnostics"): host samples [chains, n, dim] */
inline std::vector<float> rank_normalize(const std::vector<float> &sample, size_t chains, size_t n, size_t dim,
                                         bool folded = false, std::vector<uint32_t> *rank2 = nullptr, int device = 0)
{
    std::vector<float> z(chains * n * dim);
    if (rank2)
        rank2->resize(z.size());
    check(mmcmc_rank_normalize(sample.data(), 0, MMCMC_F32, chains, n, dim, folded ? 1 : 0, z.data(), 0,
                               rank2 ? rank2->data() : nullptr, device, nullptr),
          "mmcmc_rank_normalize");
    return z;
}
/* [probs.size(), dim], numpy's default rule */
inline std::vector<double> quantiles(const std::vector<float> &sample, size_t chains, size_t n, size_t dim,
                                     const std::vector<double> &probs, int device = 0)
{
    std::vector<double> out(probs.size() * dim);
    check(mmcmc_quantiles(sample.data(), 0, MMCMC_F32, chains, n, dim, probs.data(), probs.size(), out.data(), device, nullptr),
          "mmcmc_quantiles");
    return out;
}
struct RankDiagnostics {
    std::vector<float> rhat, rhat_bulk, rhat_folded, ess_bulk, ess_tail, ess_tail_lower, ess_tail_upper;
    std::vector<double> quantiles; /* [probs.size(), dim] */
};
inline RankDiagnostics rank_diagnostics(const std::vector<float> &sample, size_t chains, size_t n, size_t dim,
                                        const std::vector<double> &probs = {0.05, 0.5, 0.95}, int device = 0)
{
    RankDiagnostics r;
    std::vector<float> rparts(2 * dim), tparts(2 * dim);
    r.rhat.resize(dim);
    r.ess_bulk.resize(dim);
    r.ess_tail.resize(dim);
    r.quantiles.resize(probs.size() * dim);
    check(mmcmc_rank_diagnostics(sample.data(), 0, MMCMC_F32, chains, n, dim, r.rhat.data(), rparts.data(), r.ess_bulk.data(),
                                 r.ess_tail.data(), tparts.data(), probs.empty() ? nullptr : probs.data(), probs.size(),
                                 probs.empty() ? nullptr : r.quantiles.data(), device, nullptr),
          "mmcmc_rank_diagnostics");
    r.rhat_bulk.assign(rparts.begin(), rparts.begin() + dim);
    r.rhat_folded.assign(rparts.begin() + dim, rparts.end());
    r.ess_tail_lower.assign(tparts.begin(), tparts.begin() + dim);
    r.ess_tail_upper.assign(tparts.begin() + dim, tparts.end());
    return r;
}

/* MultiChainTracker (stats.rs:189-306): step() takes host states [n_chains, k, dim] */
class MultiChainTracker {
    mmcmc_tracker *h_ = nullptr;
    size_t n_chains_, dim_;

  public:
    MultiChainTracker(size_t n_chains, size_t n_params, int device = 0) : n_chains_(n_chains), dim_(n_params)
    {
        check(mmcmc_tracker_create(&h_, n_chains, n_params, device), "mmcmc_tracker_create");
    }
    /* own a tracker the library handed back (mmcmc_*_run_progress' tracker_out) */
    explicit MultiChainTracker(mmcmc_tracker *adopt) : h_(adopt), n_chains_(0), dim_(0)
    {
        check(mmcmc_tracker_shape(h_, &n_chains_, &dim_, nullptr), "mmcmc_tracker_shape");
    }
    MultiChainTracker(const MultiChainTracker &) = delete;
    MultiChainTracker &operator=(const MultiChainTracker &) = delete;
    ~MultiChainTracker() { mmcmc_tracker_destroy(h_); }
    template <class T> void step(const std::vector<T> &states)
    {
        const size_t k = states.size() / (n_chains_ * dim_);
        check(mmcmc_tracker_steps(h_, states.data(), 0, dtype_of<T>(), k, 0, k, nullptr), "mmcmc_tracker_steps");
    }
    std::vector<float> rhat()
    {
        std::vector<float> r(dim_);
        check(mmcmc_tracker_stats(h_, r.data(), nullptr, nullptr, nullptr), "mmcmc_tracker_stats");
        return r;
    }
    float max_rhat()
    {
        float m = 0.f;
        check(mmcmc_tracker_stats(h_, nullptr, &m, nullptr, nullptr), "mmcmc_tracker_stats");
        return m;
    }
    float p_accept()
    {
        float p = 0.f;
        check(mmcmc_tracker_stats(h_, nullptr, nullptr, &p, nullptr), "mmcmc_tracker_stats");
        return p;
    }
    /* the per-chain flavour (ChainTracker + collect_rhat, stats.rs:26-178): rhat [dim]; max_rhat / avg_p_accept may be NULL */
    std::vector<float> chain_rhat(float *max_rhat = nullptr, float *avg_p_accept = nullptr)
    {
        std::vector<float> r(dim_);
        check(mmcmc_tracker_chain_stats(h_, r.data(), max_rhat, avg_p_accept, nullptr), "mmcmc_tracker_chain_stats");
        return r;
    }
    uint64_t n() const
    {
        uint64_t v = 0;
        check(mmcmc_tracker_n(h_, &v), "mmcmc_tracker_n");
        return v;
    }
    mmcmc_tracker *handle() const { return h_; }
};

/* stats::ess_from_chainstats (stats.rs:668-671): un-split ESS of sample [chains, n, dim] with the per-chain trackers' within / var */
inline std::vector<float> ess_from_chainstats(const std::vector<float> &sample, size_t chains, size_t n, size_t dim,
                                              const MultiChainTracker &tracker, int device = 0)
{
    std::vector<float> ess(dim);
    check(mmcmc_ess_from_chainstats(sample.data(), 0, MMCMC_F32, chains, n, dim, tracker.handle(), ess.data(), device, nullptr),
          "mmcmc_ess_from_chainstats");
    return ess;
}

/* what run_progress returns: (sample [n_chains, n_collect, dim], RunStats) as the reference, plus the tracker that was fed */
template <class T> struct ProgressResult {
    std::vector<T> sample;
    RunStats stats;
    std::unique_ptr<MultiChainTracker> tracker;
};



/* ---- MetropolisHastings<T> ---- */
template <class T> class MetropolisHastings {
    mmcmc_mh *h_ = nullptr;
    size_t n_chains_, dim_;

  public:
    /* MetropolisHastings::new(target, proposal, initial_states); initial_states row-major [n_chains, dim] */
    MetropolisHastings(Target target, IsotropicGaussian proposal, const std::vector<T> &initial_states, size_t n_chains,
                       int device = 0)
        : n_chains_(n_chains), dim_(initial_states.size() / n_chains)
    {
        mmcmc_proposal_desc p{MMCMC_PROPOSAL_ISOTROPIC_GAUSSIAN, 0, proposal.std};
        check(mmcmc_mh_create(&h_, target.desc(), &p, initial_states.data(), n_chains, dtype_of<T>(), device),
              "mmcmc_mh_create");
    }
    MetropolisHastings(const MetropolisHastings &) = delete;
    MetropolisHastings &operator=(const MetropolisHastings &) = delete;
    ~MetropolisHastings() { mmcmc_mh_destroy(h_); }
    MetropolisHastings &seed(uint64_t s)
    {
        check(mmcmc_mh_seed(h_, s), "mmcmc_mh_seed");
        return *this;
    }
    /* ChainRunner::run -> [n_chains, n_collect, dim] */
    std::vector<T> run(size_t n_collect, size_t n_discard, std::vector<uint64_t> *accept_counts = nullptr)
    {
        std::vector<T> out(n_chains_ * n_collect * dim_);
        if (accept_counts)
            accept_counts->assign(n_chains_, 0);
        check(mmcmc_mh_run(h_, n_collect, n_discard, out.data(), 0, accept_counts ? accept_counts->data() : nullptr,
                           nullptr),
              "mmcmc_mh_run");
        check(mmcmc_mh_sync(h_), "mmcmc_mh_sync");
        return out;
    }
    size_t n_chains() const { return n_chains_; }
    size_t dim() const { return dim_; }
    /* the reference's public fields (metropolis_hastings.rs:101-109): from the next transition on */
    MetropolisHastings &set_proposal_std(double std)
    {
        check(mmcmc_mh_set_proposal_std(h_, std), "mmcmc_mh_set_proposal_std");
        return *this;
    }
    double proposal_std()
    {
        double std = 0;
        check(mmcmc_mh_params(h_, &std), "mmcmc_mh_params");
        return std;
    }
    std::vector<T> positions()
    {
        std::vector<T> out(n_chains_ * dim_);
        check(mmcmc_mh_state(h_, out.data()), "mmcmc_mh_state");
        return out;
    }
    MetropolisHastings &set_positions(const std::vector<T> &positions)
    {
        if (positions.size() != n_chains_ * dim_)
            throw Error(MMCMC_ERR_SHAPE, "MetropolisHastings::set_positions");
        check(mmcmc_mh_set_state(h_, positions.data(), 0, nullptr), "mmcmc_mh_set_state");
        return *this;
    }
    StreamPosition stream_position()
    {
        StreamPosition p;
        check(mmcmc_mh_stream_position(h_, &p.seed, &p.chain_offset, &p.iteration), "mmcmc_mh_stream_position");
        return p;
    }
    MetropolisHastings &set_iteration(uint64_t iteration)
    {
        check(mmcmc_mh_set_iteration(h_, iteration), "mmcmc_mh_set_iteration");
        return *this;
    }
    /* ChainRunner::run_progress (core.rs:208-360): cb(user, done, total, p_accept, max_rhat) after every `every` transitions */
    ProgressResult<T> run_progress(size_t n_collect, size_t n_discard, size_t every = 0, mmcmc_progress_fn cb = nullptr,
                                   void *user = nullptr)
    {
        ProgressResult<T> r;
        r.sample.resize(n_chains_ * n_collect * dim_);
        mmcmc_tracker *t = nullptr;
        check(mmcmc_mh_run_progress(h_, n_collect, n_discard, every, cb, user, r.sample.data(), 0, &r.stats.s, &t, nullptr),
              "mmcmc_mh_run_progress");
        r.tracker.reset(new MultiChainTracker(t));
        return r;
    }
};

/* ---- HMC<T> ---- */
template <class T> class HMC {
    mmcmc_hmc *h_ = nullptr;
    size_t n_chains_, dim_;

  public:
    HMC(Target target, const std::vector<T> &initial_positions, size_t n_chains, T step_size, int n_leapfrog,
        int device = 0)
        : n_chains_(n_chains), dim_(initial_positions.size() / n_chains)
    {
        check(mmcmc_hmc_create(&h_, target.desc(), initial_positions.data(), n_chains, (double)step_size, n_leapfrog,
                               dtype_of<T>(), device),
              "mmcmc_hmc_create");
    }
    HMC(const HMC &) = delete;
    HMC &operator=(const HMC &) = delete;
    ~HMC() { mmcmc_hmc_destroy(h_); }
    HMC &set_seed(uint64_t s)
    {
        check(mmcmc_hmc_seed(h_, s), "mmcmc_hmc_seed");
        return *this;
    }
    std::vector<T> run(size_t n_collect, size_t n_discard)
    {
        std::vector<T> out(n_chains_ * n_collect * dim_);
        check(mmcmc_hmc_run(h_, n_collect, n_discard, out.data(), 0, nullptr, nullptr), "mmcmc_hmc_run");
        check(mmcmc_hmc_sync(h_), "mmcmc_hmc_sync");
        return out;
    }
    /* HMC::run_progress (hmc.rs:222-294) */
    ProgressResult<T> run_progress(size_t n_collect, size_t n_discard, size_t every = 0, mmcmc_progress_fn cb = nullptr,
                                   void *user = nullptr)
    {
        ProgressResult<T> r;
        r.sample.resize(n_chains_ * n_collect * dim_);
        mmcmc_tracker *t = nullptr;
        check(mmcmc_hmc_run_progress(h_, n_collect, n_discard, every, cb, user, r.sample.data(), 0, &r.stats.s, &t, nullptr),
              "mmcmc_hmc_run_progress");
        r.tracker.reset(new MultiChainTracker(t));
        return r;
    }
    void step()
    {
        check(mmcmc_hmc_step(h_, nullptr), "mmcmc_hmc_step");
        check(mmcmc_hmc_sync(h_), "mmcmc_hmc_sync");
    }
    std::vector<T> positions()
    {
        std::vector<T> out(n_chains_ * dim_);
        check(mmcmc_hmc_state(h_, out.data()), "mmcmc_hmc_state");
        return out;
    }
    /* the reference's public fields (hmc.rs:41-49): from the next transition on */
    HMC &set_step_size(double step_size)
    {
        check(mmcmc_hmc_set_step_size(h_, step_size), "mmcmc_hmc_set_step_size");
        return *this;
    }
    HMC &set_n_leapfrog(int n_leapfrog)
    {
        check(mmcmc_hmc_set_n_leapfrog(h_, n_leapfrog), "mmcmc_hmc_set_n_leapfrog");
        return *this;
    }
    /* the diagonal metric (mmcmc_hmc_set_metric): a scale per coordinate, or clear_metric() for the identity */
    HMC &set_metric(const std::vector<double> &scale)
    {
        if (scale.size() != dim_)
            throw Error(MMCMC_ERR_SHAPE, "HMC::set_metric");
        check(mmcmc_hmc_set_metric(h_, scale.data()), "mmcmc_hmc_set_metric");
        return *this;
    }
    HMC &clear_metric()
    {
        check(mmcmc_hmc_set_metric(h_, nullptr), "mmcmc_hmc_set_metric");
        return *this;
    }
    /* the scales last set, ones when none is; *is_set (may be NULL) tells which */
    std::vector<double> metric(bool *is_set = nullptr)
    {
        std::vector<double> out(dim_);
        const int st = mmcmc_hmc_metric(h_, out.data());
        if (st < 0)
            check(st, "mmcmc_hmc_metric");
        if (is_set)
            *is_set = st == 1; /* 2: a dense metric is set (metric_dense()), and these are the row norms of its factor */
        return out;
    }
    /* the dense metric (mmcmc_hmc_set_metric_dense): a lower-triangular factor L, row-major [dim, dim], Sigma = L L^T; it
     * replaces a diagonal metric, and clear_metric() removes either */
    HMC &set_metric_dense(const std::vector<double> &chol)
    {
        if (chol.size() != dim_ * dim_)
            throw Error(MMCMC_ERR_SHAPE, "HMC::set_metric_dense");
        check(mmcmc_hmc_set_metric_dense(h_, chol.data()), "mmcmc_hmc_set_metric_dense");
        return *this;
    }
    /* the factor last set, empty when no dense metric is set */
    std::vector<double> metric_dense()
    {
        std::vector<double> out(dim_ * dim_);
        const int st = mmcmc_hmc_metric_dense(h_, out.data());
        if (st < 0)
            check(st, "mmcmc_hmc_metric_dense");
        if (st == 0)
            out.clear();
        return out;
    }
    double step_size()
    {
        double eps = 0;
        check(mmcmc_hmc_params(h_, &eps, nullptr), "mmcmc_hmc_params");
        return eps;
    }
    int n_leapfrog()
    {
        int n = 0;
        check(mmcmc_hmc_params(h_, nullptr, &n), "mmcmc_hmc_params");
        return n;
    }
    HMC &set_positions(const std::vector<T> &positions)
    {
        if (positions.size() != n_chains_ * dim_)
            throw Error(MMCMC_ERR_SHAPE, "HMC::set_positions");
        check(mmcmc_hmc_set_state(h_, positions.data(), 0, nullptr), "mmcmc_hmc_set_state");
        return *this;
    }
    StreamPosition stream_position()
    {
        StreamPosition p;
        check(mmcmc_hmc_stream_position(h_, &p.seed, &p.chain_offset, &p.iteration), "mmcmc_hmc_stream_position");
        return p;
    }
    HMC &set_iteration(uint64_t iteration)
    {
        check(mmcmc_hmc_set_iteration(h_, iteration), "mmcmc_hmc_set_iteration");
        return *this;
    }
    /* transition k uses (step_sizes[k], n_leapfrogs[k]), the first size - n_collect are discarded: the loop
     * set_step_size; set_n_leapfrog; step() bit for bit, in one call */
    std::vector<T> run_scheduled(const std::vector<double> &step_sizes, const std::vector<int32_t> &n_leapfrogs, size_t n_collect)
    {
        if (step_sizes.size() != n_leapfrogs.size() || n_collect > step_sizes.size())
            throw Error(MMCMC_ERR_INVALID_ARG, "HMC::run_scheduled");
        std::vector<T> out(n_chains_ * n_collect * dim_);
        check(mmcmc_hmc_run_scheduled(h_, n_collect, step_sizes.size() - n_collect, step_sizes.data(), n_leapfrogs.data(),
                                      out.data(), 0, nullptr, nullptr),
              "mmcmc_hmc_run_scheduled");
        check(mmcmc_hmc_sync(h_), "mmcmc_hmc_sync");
        return out;
    }
};

/* ---- a target of the user's own: the GPU analogue of `impl GradientTarget for MyDensity` (distributions.rs:65-108).
 * `hip_source` defines `template <class T> struct mmcmc_user_target` (dim, logp, logp_grad; include/mmcmc.h); it is
 * compiled at run time and the returned Target is accepted wherever a built-in one is (MH / HMC, dim <= 32). ---- */
namespace detail {
typedef int (*register_source_fn)(const char *, int, const char *, int *, char *, size_t);
inline Target register_target(register_source_fn fn, const char *what, const std::string &name, int dim, const std::string &source,
                              const std::vector<double> &params)
{
    int kind = 0;
    std::string log(1 << 16, '\0');
    const int st = fn(name.c_str(), dim, source.c_str(), &kind, &log[0], log.size());
    if (st != MMCMC_OK)
        throw Error(st, std::string(what) + ": " + std::string(log.c_str()));
    Target t;
    t.d.kind = kind;
    t.d.dim = dim;
    for (size_t i = 0; i < params.size() && i < 8; ++i)
        t.d.params[i] = params[i];
    return t;
}
} // namespace detail

inline Target UserTarget(const std::string &name, int dim, const std::string &hip_source, const std::vector<double> &params = {})
{
    return detail::register_target(mmcmc_target_register_source, "mmcmc_target_register_source", name, dim, hip_source, params);
}

/* ... and from its log-density alone: `logp_source` defines `template <class T> struct mmcmc_user_logp` with
 * `template <class S> S logp(P, const S *x)` (loops over the coordinates under MM_UNROLL); the gradient is forward-mode
 * automatic differentiation of that body on the device (mmcmc_target_register_logp_source, include/mmcmc.h). */
inline Target AutodiffTarget(const std::string &name, int dim, const std::string &logp_source, const std::vector<double> &params = {})
{
    return detail::register_target(mmcmc_target_register_logp_source, "mmcmc_target_register_logp_source", name, dim, logp_source, params);
}

/* ... and over DATA: the kind is registered with data.size() values (mmcmc_target_register_data_source), which the functor
 * reads as P.mat[0 .. data_len) (csrc/mm_data.h: mm_data_row) and every sampler created from the Target copies to its
 * device.  with_data(t, other) is the same compiled kind over another array of that size. */
namespace detail {
inline Target register_data_target(int flavour, const std::string &name, int dim, const std::string &source,
                                   const std::vector<double> &params, const std::vector<double> &data)
{
    int kind = 0;
    std::string log(1 << 16, '\0');
    const int st = mmcmc_target_register_data_source(name.c_str(), dim, data.size(), flavour, source.c_str(), &kind, &log[0], log.size());
    if (st != MMCMC_OK)
        throw Error(st, std::string("mmcmc_target_register_data_source: ") + std::string(log.c_str()));
    Target t;
    t.d.kind = kind;
    t.d.dim = dim;
    for (size_t i = 0; i < params.size() && i < 8; ++i)
        t.d.params[i] = params[i];
    t.matrix = data;
    return t;
}
} // namespace detail
inline Target UserTarget(const std::string &name, int dim, const std::string &hip_source, const std::vector<double> &params,
                         const std::vector<double> &data)
{
    return detail::register_data_target(MMCMC_SOURCE_LOGP_GRAD, name, dim, hip_source, params, data);
}
inline Target AutodiffTarget(const std::string &name, int dim, const std::string &logp_source, const std::vector<double> &params,
                             const std::vector<double> &data)
{
    return detail::register_data_target(MMCMC_SOURCE_LOGP, name, dim, logp_source, params, data);
}
inline Target with_data(const Target &t, const std::vector<double> &data)
{
    size_t len = 0;
    check(mmcmc_target_data_len(t.d.kind, &len), "mmcmc_target_data_len");
    if (len == 0 || data.size() != len)
        throw Error(MMCMC_ERR_INVALID_ARG, "with_data: the kind was registered with another number of values");
    Target r = t;
    r.matrix = data;
    return r;
}

/* the groups' collectives from a named library instead of librccl (mmcmc_group_bind_collectives): once per process, before
 * the first group; ranks_may_share_a_device only for a library that accepts several ranks on one device */
inline void bind_collectives(const std::string &library_path, bool ranks_may_share_a_device = false)
{
    check(mmcmc_group_bind_collectives(library_path.c_str(), ranks_may_share_a_device ? 1 : 0), "mmcmc_group_bind_collectives");
}

/* ---- HMC over several GPUs from one call: run() executes every chain (ChainRunner::run, core.rs:176-186) ---- */
template <class T> class HMCGroup {
    mmcmc_hmc_group *g_ = nullptr;
    size_t n_chains_, dim_;

  public:
    HMCGroup(Target target, const std::vector<T> &initial_positions, size_t n_chains, T step_size, int n_leapfrog,
             const std::vector<int> &devices)
        : n_chains_(n_chains), dim_(initial_positions.size() / n_chains)
    {
        check(mmcmc_hmc_group_create(&g_, target.desc(), initial_positions.data(), n_chains, (double)step_size, n_leapfrog,
                                     dtype_of<T>(), devices.data(), (int)devices.size()),
              "mmcmc_hmc_group_create");
    }
    HMCGroup(const HMCGroup &) = delete;
    HMCGroup &operator=(const HMCGroup &) = delete;
    ~HMCGroup() { mmcmc_hmc_group_destroy(g_); }
    HMCGroup &set_seed(uint64_t s)
    {
        check(mmcmc_hmc_group_seed(g_, s), "mmcmc_hmc_group_seed");
        return *this;
    }
    std::vector<T> run(size_t n_collect, size_t n_discard)
    {
        std::vector<T> out(n_chains_ * n_collect * dim_);
        check(mmcmc_hmc_group_run(g_, n_collect, n_discard, out.data(), nullptr), "mmcmc_hmc_group_run");
        return out;
    }
    /* the same run with the sample left on the devices: only ENQUEUED on the shards' streams (returns at once; several in a
     * row keep every device busy); sync() waits, split_rhat_mean_ess() orders itself behind them */
    void run_on_devices(size_t n_collect, size_t n_discard)
    {
        check(mmcmc_hmc_group_run_async(g_, n_collect, n_discard), "mmcmc_hmc_group_run_async");
    }
    void sync() { check(mmcmc_hmc_group_sync(g_), "mmcmc_hmc_group_sync"); }
    /* global [n_chains, dim], split across the shards; behind the runs queued on each shard's stream */
    HMCGroup &set_positions(const std::vector<T> &positions)
    {
        if (positions.size() != n_chains_ * dim_)
            throw Error(MMCMC_ERR_SHAPE, "HMCGroup::set_positions");
        check(mmcmc_hmc_group_set_state(g_, positions.data()), "mmcmc_hmc_group_set_state");
        return *this;
    }
    std::vector<T> positions()
    {
        std::vector<T> out(n_chains_ * dim_);
        check(mmcmc_hmc_group_state(g_, out.data()), "mmcmc_hmc_group_state");
        return out;
    }
    HMCGroup &set_step_size(double step_size)
    {
        check(mmcmc_hmc_group_set_step_size(g_, step_size), "mmcmc_hmc_group_set_step_size");
        return *this;
    }
    HMCGroup &set_n_leapfrog(int n_leapfrog)
    {
        check(mmcmc_hmc_group_set_n_leapfrog(g_, n_leapfrog), "mmcmc_hmc_group_set_n_leapfrog");
        return *this;
    }
    StreamPosition stream_position()
    {
        StreamPosition p;
        check(mmcmc_hmc_group_stream_position(g_, &p.seed, &p.chain_offset, &p.iteration), "mmcmc_hmc_group_stream_position");
        return p;
    }
    HMCGroup &set_iteration(uint64_t iteration)
    {
        check(mmcmc_hmc_group_set_iteration(g_, iteration), "mmcmc_hmc_group_set_iteration");
        return *this;
    }
    /* how the diagnostics will travel (1 RCCL, 0 host by design, < 0 host as a fallback), known from construction on */
    int exchange() const
    {
        int status = 0;
        check(mmcmc_hmc_group_exchange(g_, &status, nullptr), "mmcmc_hmc_group_exchange");
        return status;
    }
    /* stats::split_rhat_mean_ess of the last run over the chains of all devices (RCCL inside the library) */
    std::pair<std::vector<float>, std::vector<float>> split_rhat_mean_ess()
    {
        std::vector<float> rhat(dim_), ess(dim_);
        check(mmcmc_hmc_group_split_rhat_mean_ess(g_, rhat.data(), ess.data(), nullptr), "mmcmc_hmc_group_split_rhat_mean_ess");
        return {rhat, ess};
    }
};

/* ---- NUTS: tensors f32, scalars T (mode 0 for T = double, 1 for T = float), like the reference backend ---- */
template <class T> class NUTS {
    mmcmc_nuts *h_ = nullptr;
    size_t n_chains_, dim_;

  public:
    NUTS(Target target, const std::vector<T> &initial_positions, size_t n_chains, T target_accept_p, int device = 0)
        : n_chains_(n_chains), dim_(initial_positions.size() / n_chains)
    {
        std::vector<double> init(initial_positions.begin(), initial_positions.end());
        check(mmcmc_nuts_create(&h_, target.desc(), init.data(), n_chains, (double)target_accept_p,
                                std::is_same<T, double>::value ? 0 : 1, device),
              "mmcmc_nuts_create");
    }
    NUTS(const NUTS &) = delete;
    NUTS &operator=(const NUTS &) = delete;
    ~NUTS() { mmcmc_nuts_destroy(h_); }
    NUTS &set_seed(uint64_t s)
    {
        check(mmcmc_nuts_seed(h_, s), "mmcmc_nuts_seed");
        return *this;
    }
    /* NUTSChain's public state (nuts.rs:361-386): position [n_chains, dim] and the adaptation records [n_chains, 4] =
     * epsilon, epsilon_bar, h_bar, mu; from the next run on */
    std::vector<float> positions()
    {
        std::vector<float> out(n_chains_ * dim_);
        check(mmcmc_nuts_state(h_, out.data()), "mmcmc_nuts_state");
        return out;
    }
    NUTS &set_positions(const std::vector<float> &positions)
    {
        if (positions.size() != n_chains_ * dim_)
            throw Error(MMCMC_ERR_SHAPE, "NUTS::set_positions");
        check(mmcmc_nuts_set_state(h_, positions.data(), 0, nullptr), "mmcmc_nuts_set_state");
        return *this;
    }
    std::vector<double> adapt_state()
    {
        std::vector<double> out(n_chains_ * 4);
        check(mmcmc_nuts_adapt_state(h_, out.data()), "mmcmc_nuts_adapt_state");
        return out;
    }
    NUTS &set_adapt_state(const std::vector<double> &adapt)
    {
        if (adapt.size() != n_chains_ * 4)
            throw Error(MMCMC_ERR_SHAPE, "NUTS::set_adapt_state");
        check(mmcmc_nuts_set_adapt_state(h_, adapt.data()), "mmcmc_nuts_set_adapt_state");
        return *this;
    }
    /* the diagonal metric (mmcmc_nuts_set_metric): a scale per coordinate, or clear_metric() for the identity */
    NUTS &set_metric(const std::vector<double> &scale)
    {
        if (scale.size() != dim_)
            throw Error(MMCMC_ERR_SHAPE, "NUTS::set_metric");
        check(mmcmc_nuts_set_metric(h_, scale.data()), "mmcmc_nuts_set_metric");
        return *this;
    }
    NUTS &clear_metric()
    {
        check(mmcmc_nuts_set_metric(h_, nullptr), "mmcmc_nuts_set_metric");
        return *this;
    }
    std::vector<double> metric(bool *is_set = nullptr)
    {
        std::vector<double> out(dim_);
        const int st = mmcmc_nuts_metric(h_, out.data());
        if (st < 0)
            check(st, "mmcmc_nuts_metric");
        if (is_set)
            *is_set = st == 1; /* 2: a dense metric is set (metric_dense()), and these are the row norms of its factor */
        return out;
    }
    /* the dense metric (mmcmc_nuts_set_metric_dense): a lower-triangular factor L, row-major [dim, dim], Sigma = L L^T; it
     * replaces a diagonal metric, and clear_metric() removes either */
    NUTS &set_metric_dense(const std::vector<double> &chol)
    {
        if (chol.size() != dim_ * dim_)
            throw Error(MMCMC_ERR_SHAPE, "NUTS::set_metric_dense");
        check(mmcmc_nuts_set_metric_dense(h_, chol.data()), "mmcmc_nuts_set_metric_dense");
        return *this;
    }
    /* the factor last set, empty when no dense metric is set */
    std::vector<double> metric_dense()
    {
        std::vector<double> out(dim_ * dim_);
        const int st = mmcmc_nuts_metric_dense(h_, out.data());
        if (st < 0)
            check(st, "mmcmc_nuts_metric_dense");
        if (st == 0)
            out.clear();
        return out;
    }
    StreamPosition stream_position()
    {
        StreamPosition p;
        check(mmcmc_nuts_stream_position(h_, &p.seed, &p.chain_offset, &p.iteration), "mmcmc_nuts_stream_position");
        return p;
    }
    NUTS &set_iteration(uint64_t iteration)
    {
        check(mmcmc_nuts_set_iteration(h_, iteration), "mmcmc_nuts_set_iteration");
        return *this;
    }
    /* per-draw statistics (mmcmc_nuts_set_draw_stats): one mmcmc_nuts_draw per chain and sample row from the next run on; no
     * result changes.  draw_stats(): the records of the last run, [n_chains, n_rows] with n_rows in *n_rows_out;
     * draw_summary(): their per-chain summary (mmcmc_nuts_draw_summary) */
    NUTS &set_draw_stats(bool on = true)
    {
        check(mmcmc_nuts_set_draw_stats(h_, on ? 1 : 0), "mmcmc_nuts_set_draw_stats");
        return *this;
    }
    bool draw_stats_enabled() { return mmcmc_nuts_draw_stats_enabled(h_) == 1; }
    std::vector<mmcmc_nuts_draw> draw_stats(size_t *n_rows_out = nullptr)
    {
        size_t n_rows = 0;
        check(mmcmc_nuts_draw_stats(h_, nullptr, 0, &n_rows), "mmcmc_nuts_draw_stats");
        std::vector<mmcmc_nuts_draw> out(n_chains_ * n_rows);
        check(mmcmc_nuts_draw_stats(h_, out.data(), 0, nullptr), "mmcmc_nuts_draw_stats");
        if (n_rows_out)
            *n_rows_out = n_rows;
        return out;
    }
    std::vector<mmcmc_nuts_chain_summary> draw_summary(int device = 0)
    {
        size_t n_rows = 0;
        const std::vector<mmcmc_nuts_draw> rec = draw_stats(&n_rows);
        std::vector<mmcmc_nuts_chain_summary> out(n_chains_);
        check(mmcmc_nuts_draw_summary(rec.data(), 0, n_chains_, n_rows, device, out.data()), "mmcmc_nuts_draw_summary");
        return out;
    }
    /* NUTS::run -> [n_chains, n_collect, dim] (f32, the backend's element type) */
    std::vector<float> run(size_t n_collect, size_t n_discard)
    {
        std::vector<float> out(n_chains_ * n_collect * dim_);
        check(mmcmc_nuts_run(h_, n_collect, n_discard, out.data(), 0, 0, nullptr), "mmcmc_nuts_run");
        check(mmcmc_nuts_sync(h_), "mmcmc_nuts_sync");
        return out;
    }
    /* NUTS::run_progress (nuts.rs:172-345): all N transitions; the per-chain trackers saw the initial position and every state */
    ProgressResult<float> run_progress(size_t n_collect, size_t n_discard, size_t every = 0, mmcmc_progress_fn cb = nullptr,
                                   void *user = nullptr)
    {
        ProgressResult<float> r;
        r.sample.resize(n_chains_ * n_collect * dim_);
        mmcmc_tracker *t = nullptr;
        check(mmcmc_nuts_run_progress(h_, n_collect, n_discard, every, cb, user, r.sample.data(), 0, &r.stats.s, &t, nullptr),
              "mmcmc_nuts_run_progress");
        r.tracker.reset(new MultiChainTracker(t));
        return r;
    }
};

/* NUTS over several GPUs from one call (mmcmc_nuts_group_*): tensors f32, scalars T, like NUTS<T> */
template <class T> class NUTSGroup {
    mmcmc_nuts_group *g_ = nullptr;
    size_t n_chains_, dim_;

  public:
    NUTSGroup(Target target, const std::vector<T> &initial_positions, size_t n_chains, T target_accept_p, const std::vector<int> &devices)
        : n_chains_(n_chains), dim_(initial_positions.size() / n_chains)
    {
        std::vector<double> init(initial_positions.begin(), initial_positions.end());
        check(mmcmc_nuts_group_create(&g_, target.desc(), init.data(), n_chains, (double)target_accept_p,
                                      std::is_same<T, double>::value ? 0 : 1, devices.data(), (int)devices.size()),
              "mmcmc_nuts_group_create");
    }
    NUTSGroup(const NUTSGroup &) = delete;
    NUTSGroup &operator=(const NUTSGroup &) = delete;
    ~NUTSGroup() { mmcmc_nuts_group_destroy(g_); }
    NUTSGroup &set_seed(uint64_t s)
    {
        check(mmcmc_nuts_group_seed(g_, s), "mmcmc_nuts_group_seed");
        return *this;
    }
    /* NUTSChain's public state (nuts.rs:361-386): position [n_chains, dim] and the adaptation records [n_chains, 4] =
     * epsilon, epsilon_bar, h_bar, mu; from the next run on */
    std::vector<float> positions()
    {
        std::vector<float> out(n_chains_ * dim_);
        check(mmcmc_nuts_group_state(g_, out.data()), "mmcmc_nuts_group_state");
        return out;
    }
    NUTSGroup &set_positions(const std::vector<float> &positions)
    {
        if (positions.size() != n_chains_ * dim_)
            throw Error(MMCMC_ERR_SHAPE, "NUTSGroup::set_positions");
        check(mmcmc_nuts_group_set_state(g_, positions.data()), "mmcmc_nuts_group_set_state");
        return *this;
    }
    std::vector<double> adapt_state()
    {
        std::vector<double> out(n_chains_ * 4);
        check(mmcmc_nuts_group_adapt_state(g_, out.data()), "mmcmc_nuts_group_adapt_state");
        return out;
    }
    NUTSGroup &set_adapt_state(const std::vector<double> &adapt)
    {
        if (adapt.size() != n_chains_ * 4)
            throw Error(MMCMC_ERR_SHAPE, "NUTSGroup::set_adapt_state");
        check(mmcmc_nuts_group_set_adapt_state(g_, adapt.data()), "mmcmc_nuts_group_set_adapt_state");
        return *this;
    }
    StreamPosition stream_position()
    {
        StreamPosition p;
        check(mmcmc_nuts_group_stream_position(g_, &p.seed, &p.chain_offset, &p.iteration), "mmcmc_nuts_group_stream_position");
        return p;
    }
    NUTSGroup &set_iteration(uint64_t iteration)
    {
        check(mmcmc_nuts_group_set_iteration(g_, iteration), "mmcmc_nuts_group_set_iteration");
        return *this;
    }
    std::vector<float> run(size_t n_collect, size_t n_discard)
    {
        std::vector<float> out(n_chains_ * n_collect * dim_);
        check(mmcmc_nuts_group_run(g_, n_collect, n_discard, out.data(), 0), "mmcmc_nuts_group_run");
        return out;
    }
    std::pair<std::vector<float>, std::vector<float>> split_rhat_mean_ess()
    {
        std::vector<float> rhat(dim_), ess(dim_);
        check(mmcmc_nuts_group_split_rhat_mean_ess(g_, rhat.data(), ess.data(), nullptr), "mmcmc_nuts_group_split_rhat_mean_ess");
        return {rhat, ess};
    }
};

/* NUTS in f64 tensors / f64 scalars (mode 2 of the C ABI; BASELINE.json config 5): for mmcmc::GaussianND of dim 16
 * or 32 this runs the lane-group / MFMA kernel with tree-depth compaction (include/mmcmc.h, kernel variants). */
class NUTS64 {
    mmcmc_nuts *h_ = nullptr;
    size_t n_chains_, dim_;

  public:
    NUTS64(Target target, const std::vector<double> &initial_positions, size_t n_chains, double target_accept_p,
           int device = 0)
        : n_chains_(n_chains), dim_(initial_positions.size() / n_chains)
    {
        check(mmcmc_nuts_create(&h_, target.desc(), initial_positions.data(), n_chains, target_accept_p, 2, device),
              "mmcmc_nuts_create");
    }
    NUTS64(const NUTS64 &) = delete;
    NUTS64 &operator=(const NUTS64 &) = delete;
    ~NUTS64() { mmcmc_nuts_destroy(h_); }
    NUTS64 &set_seed(uint64_t s)
    {
        check(mmcmc_nuts_seed(h_, s), "mmcmc_nuts_seed");
        return *this;
    }
    /* NUTSChain's public state (nuts.rs:361-386): position [n_chains, dim] and the adaptation records [n_chains, 4] =
     * epsilon, epsilon_bar, h_bar, mu; from the next run on */
    std::vector<double> positions()
    {
        std::vector<double> out(n_chains_ * dim_);
        check(mmcmc_nuts_state(h_, out.data()), "mmcmc_nuts_state");
        return out;
    }
    NUTS64 &set_positions(const std::vector<double> &positions)
    {
        if (positions.size() != n_chains_ * dim_)
            throw Error(MMCMC_ERR_SHAPE, "NUTS64::set_positions");
        check(mmcmc_nuts_set_state(h_, positions.data(), 0, nullptr), "mmcmc_nuts_set_state");
        return *this;
    }
    std::vector<double> adapt_state()
    {
        std::vector<double> out(n_chains_ * 4);
        check(mmcmc_nuts_adapt_state(h_, out.data()), "mmcmc_nuts_adapt_state");
        return out;
    }
    NUTS64 &set_adapt_state(const std::vector<double> &adapt)
    {
        if (adapt.size() != n_chains_ * 4)
            throw Error(MMCMC_ERR_SHAPE, "NUTS64::set_adapt_state");
        check(mmcmc_nuts_set_adapt_state(h_, adapt.data()), "mmcmc_nuts_set_adapt_state");
        return *this;
    }
    /* the diagonal metric (mmcmc_nuts_set_metric): a scale per coordinate, or clear_metric() for the identity */
    NUTS64 &set_metric(const std::vector<double> &scale)
    {
        if (scale.size() != dim_)
            throw Error(MMCMC_ERR_SHAPE, "NUTS64::set_metric");
        check(mmcmc_nuts_set_metric(h_, scale.data()), "mmcmc_nuts_set_metric");
        return *this;
    }
    NUTS64 &clear_metric()
    {
        check(mmcmc_nuts_set_metric(h_, nullptr), "mmcmc_nuts_set_metric");
        return *this;
    }
    std::vector<double> metric(bool *is_set = nullptr)
    {
        std::vector<double> out(dim_);
        const int st = mmcmc_nuts_metric(h_, out.data());
        if (st < 0)
            check(st, "mmcmc_nuts_metric");
        if (is_set)
            *is_set = st == 1; /* 2: a dense metric is set (metric_dense()), and these are the row norms of its factor */
        return out;
    }
    /* the dense metric (mmcmc_nuts_set_metric_dense): a lower-triangular factor L, row-major [dim, dim], Sigma = L L^T; it
     * replaces a diagonal metric, and clear_metric() removes either */
    NUTS64 &set_metric_dense(const std::vector<double> &chol)
    {
        if (chol.size() != dim_ * dim_)
            throw Error(MMCMC_ERR_SHAPE, "NUTS64::set_metric_dense");
        check(mmcmc_nuts_set_metric_dense(h_, chol.data()), "mmcmc_nuts_set_metric_dense");
        return *this;
    }
    /* the factor last set, empty when no dense metric is set */
    std::vector<double> metric_dense()
    {
        std::vector<double> out(dim_ * dim_);
        const int st = mmcmc_nuts_metric_dense(h_, out.data());
        if (st < 0)
            check(st, "mmcmc_nuts_metric_dense");
        if (st == 0)
            out.clear();
        return out;
    }
    StreamPosition stream_position()
    {
        StreamPosition p;
        check(mmcmc_nuts_stream_position(h_, &p.seed, &p.chain_offset, &p.iteration), "mmcmc_nuts_stream_position");
        return p;
    }
    NUTS64 &set_iteration(uint64_t iteration)
    {
        check(mmcmc_nuts_set_iteration(h_, iteration), "mmcmc_nuts_set_iteration");
        return *this;
    }
    /* per-draw statistics (mmcmc_nuts_set_draw_stats): one mmcmc_nuts_draw per chain and sample row from the next run on; no
     * result changes.  draw_stats(): the records of the last run, [n_chains, n_rows] with n_rows in *n_rows_out;
     * draw_summary(): their per-chain summary (mmcmc_nuts_draw_summary) */
    NUTS64 &set_draw_stats(bool on = true)
    {
        check(mmcmc_nuts_set_draw_stats(h_, on ? 1 : 0), "mmcmc_nuts_set_draw_stats");
        return *this;
    }
    bool draw_stats_enabled() { return mmcmc_nuts_draw_stats_enabled(h_) == 1; }
    std::vector<mmcmc_nuts_draw> draw_stats(size_t *n_rows_out = nullptr)
    {
        size_t n_rows = 0;
        check(mmcmc_nuts_draw_stats(h_, nullptr, 0, &n_rows), "mmcmc_nuts_draw_stats");
        std::vector<mmcmc_nuts_draw> out(n_chains_ * n_rows);
        check(mmcmc_nuts_draw_stats(h_, out.data(), 0, nullptr), "mmcmc_nuts_draw_stats");
        if (n_rows_out)
            *n_rows_out = n_rows;
        return out;
    }
    std::vector<mmcmc_nuts_chain_summary> draw_summary(int device = 0)
    {
        size_t n_rows = 0;
        const std::vector<mmcmc_nuts_draw> rec = draw_stats(&n_rows);
        std::vector<mmcmc_nuts_chain_summary> out(n_chains_);
        check(mmcmc_nuts_draw_summary(rec.data(), 0, n_chains_, n_rows, device, out.data()), "mmcmc_nuts_draw_summary");
        return out;
    }
    NUTS64 &set_max_depth(int d)
    {
        check(mmcmc_nuts_set_max_depth(h_, d), "mmcmc_nuts_set_max_depth");
        return *this;
    }
    NUTS64 &set_kernel_variant(int v)
    {
        check(mmcmc_nuts_set_kernel_variant(h_, v), "mmcmc_nuts_set_kernel_variant");
        return *this;
    }
    int kernel_variant() const { return mmcmc_nuts_kernel_variant(h_); }
    std::vector<double> run(size_t n_collect, size_t n_discard)
    {
        std::vector<double> out(n_chains_ * n_collect * dim_);
        check(mmcmc_nuts_run(h_, n_collect, n_discard, out.data(), 0, 0, nullptr), "mmcmc_nuts_run");
        check(mmcmc_nuts_sync(h_), "mmcmc_nuts_sync");
        return out;
    }
    /* NUTS::run_progress (nuts.rs:172-345): all N transitions; the per-chain trackers saw the initial position and every state */
    ProgressResult<double> run_progress(size_t n_collect, size_t n_discard, size_t every = 0, mmcmc_progress_fn cb = nullptr,
                                   void *user = nullptr)
    {
        ProgressResult<double> r;
        r.sample.resize(n_chains_ * n_collect * dim_);
        mmcmc_tracker *t = nullptr;
        check(mmcmc_nuts_run_progress(h_, n_collect, n_discard, every, cb, user, r.sample.data(), 0, &r.stats.s, &t, nullptr),
              "mmcmc_nuts_run_progress");
        r.tracker.reset(new MultiChainTracker(t));
        return r;
    }
};

/* MetropolisHastings<i32, f64, ...> over the reference's discrete test models (include/mmcmc.h: MMCMC_POISSON_REFLECT,
 * MMCMC_BINOMIAL_CLAMP, MMCMC_POISSON_NONNEG); run() -> [n_chains, n_collect] */
class DiscreteMetropolisHastings {
    mmcmc_mh_discrete *h_ = nullptr;
    size_t n_chains_;

  public:
    DiscreteMetropolisHastings(int kind, const std::vector<double> &params, const std::vector<int32_t> &initial_states,
                               int device = 0)
        : n_chains_(initial_states.size())
    {
        check(mmcmc_mh_discrete_create(&h_, kind, params.data(), initial_states.data(), n_chains_, device),
              "mmcmc_mh_discrete_create");
    }
    DiscreteMetropolisHastings(const DiscreteMetropolisHastings &) = delete;
    DiscreteMetropolisHastings &operator=(const DiscreteMetropolisHastings &) = delete;
    ~DiscreteMetropolisHastings() { mmcmc_mh_discrete_destroy(h_); }
    DiscreteMetropolisHastings &seed(uint64_t s)
    {
        check(mmcmc_mh_discrete_seed(h_, s), "mmcmc_mh_discrete_seed");
        return *this;
    }
    /* MHMarkovChain::current_state of every chain [n_chains]: from the next run on */
    DiscreteMetropolisHastings &set_state(const std::vector<int32_t> &states)
    {
        if (states.size() != n_chains_)
            throw Error(MMCMC_ERR_SHAPE, "DiscreteMetropolisHastings::set_state");
        check(mmcmc_mh_discrete_set_state(h_, states.data()), "mmcmc_mh_discrete_set_state");
        return *this;
    }
    StreamPosition stream_position()
    {
        StreamPosition p;
        check(mmcmc_mh_discrete_stream_position(h_, &p.seed, &p.chain_offset, &p.iteration), "mmcmc_mh_discrete_stream_position");
        return p;
    }
    DiscreteMetropolisHastings &set_iteration(uint64_t iteration)
    {
        check(mmcmc_mh_discrete_set_iteration(h_, iteration), "mmcmc_mh_discrete_set_iteration");
        return *this;
    }
    std::vector<int32_t> run(size_t n_collect, size_t n_discard)
    {
        std::vector<int32_t> out(n_chains_ * n_collect);
        check(mmcmc_mh_discrete_run(h_, n_collect, n_discard, out.data(), 0, nullptr), "mmcmc_mh_discrete_run");
        return out;
    }
    std::vector<uint64_t> accept_counts()
    {
        std::vector<uint64_t> a(n_chains_);
        check(mmcmc_mh_discrete_accept_counts(h_, a.data()), "mmcmc_mh_discrete_accept_counts");
        return a;
    }
};

/* GibbsSampler<f64, MixtureConditional> (gibbs.rs:139-203, 231-285); run() -> [n_chains, n_collect, 2] */
class GibbsMixtureSampler {
    mmcmc_gibbs_mixture *h_ = nullptr;
    size_t n_chains_;

  public:
    GibbsMixtureSampler(double mu0, double sigma0, double mu1, double sigma1, double pi0,
                        const std::vector<double> &initial_states, int device = 0)
        : n_chains_(initial_states.size() / 2)
    {
        const double p[5] = {mu0, sigma0, mu1, sigma1, pi0};
        check(mmcmc_gibbs_mixture_create(&h_, p, initial_states.data(), n_chains_, device), "mmcmc_gibbs_mixture_create");
    }
    GibbsMixtureSampler(const GibbsMixtureSampler &) = delete;
    GibbsMixtureSampler &operator=(const GibbsMixtureSampler &) = delete;
    ~GibbsMixtureSampler() { mmcmc_gibbs_mixture_destroy(h_); }
    GibbsMixtureSampler &set_seed(uint64_t s)
    {
        check(mmcmc_gibbs_mixture_seed(h_, s), "mmcmc_gibbs_mixture_seed");
        return *this;
    }
    /* GibbsMarkovChain::current_state of every chain [n_chains, 2]: from the next run on */
    GibbsMixtureSampler &set_state(const std::vector<double> &states)
    {
        if (states.size() != n_chains_ * 2)
            throw Error(MMCMC_ERR_SHAPE, "GibbsMixtureSampler::set_state");
        check(mmcmc_gibbs_mixture_set_state(h_, states.data()), "mmcmc_gibbs_mixture_set_state");
        return *this;
    }
    StreamPosition stream_position()
    {
        StreamPosition p;
        check(mmcmc_gibbs_mixture_stream_position(h_, &p.seed, &p.chain_offset, &p.iteration), "mmcmc_gibbs_mixture_stream_position");
        return p;
    }
    GibbsMixtureSampler &set_iteration(uint64_t iteration)
    {
        check(mmcmc_gibbs_mixture_set_iteration(h_, iteration), "mmcmc_gibbs_mixture_set_iteration");
        return *this;
    }
    std::vector<double> run(size_t n_collect, size_t n_discard)
    {
        std::vector<double> out(n_chains_ * n_collect * 2);
        check(mmcmc_gibbs_mixture_run(h_, n_collect, n_discard, out.data(), 0, nullptr), "mmcmc_gibbs_mixture_run");
        return out;
    }
};

} // namespace mmcmc
#endif /* MMCMC_HPP */
