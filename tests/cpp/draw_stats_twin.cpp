/* draw_stats_twin.cpp -- NUTS's per-draw records (include/mmcmc.h: mmcmc_nuts_draw; csrc/mm_nuts.h: mm_draw_recorder) on the host.
 *
 * A plain C++17 program around the very headers the kernels are compiled from, built with the flags of oracle/Makefile
 * (-ffp-contract=off), so what it computes is what the device computes, bit for bit.
 *
 * Without arguments it checks, and exits 0 only if every check held:
 *  (1) the recorder changes nothing: RosenbrockND(3), 8 chains, 30 transitions with and without adaptation (n_discard 10
 *      and 0), the three type modes, no metric / a diagonal / a dense metric, walked leaf by leaf and in pairs -- samples,
 *      positions, adaptation records, leapfrog counts and depths of the recording policy equal the empty policy's;
 *  (2) the record is right, for every transition of those runs: n_leapfrog and depth are mm_nuts_info's; energy is the
 *      float of -(logp(x_prev) - 0.5 p0.p0), recomputed from mm_nuts_momentum and the functor in the tree's order; step_size
 *      is the float of the adaptation record's epsilon before the transition; accept_stat satisfies dual averaging's
 *      h_bar' = (1 - eta) h_bar + eta (delta - accept_stat) against a rerun of the transition under the empty policy from a
 *      saved adaptation record, to 4 ulp of ST plus, where ST is double, eta times half an ulp of the float the record
 *      holds (the record is the ST value converted once); the depth-cap bit is depth >= max_depth; the two walks give the
 *      same records; row 0 of a run without burn-in is the no-transition record;
 *  (3) divergence forced and absent: Gaussian2D with unit covariance, 96 chains x 20 rows, epsilon = epsilon_bar = 64
 *      (every transition divergent, depth 1, one leapfrog, every sample row the start) and 0.1 (no divergent bit).
 * With arguments it is the reference of the GPU tests (tests/draw_stats_common.py):
 *   draw_stats_twin nuts <mode> <chains> <n_collect> <n_discard> <progress 0|1> <seed> <none|diag|dense> <out file>   RosenbrockND(3)
 *   draw_stats_twin gauss <mode> <chains> <rows> <epsilon> <seed> <out file>                   Gaussian2D, unit covariance
 * from the fixed start x0[c][i] = 0.05 * ((7 c + 13 i) mod 17 - 8) + 0.01 i, the diagonal metric (0.37, 2.9, 11.0) and the
 * dense factor general_factor() below.  The out file holds, raw: samples [C, n_collect, D] and positions [C, D] (tensor
 * type), adaptation records [C, 4] f64, leapfrog counts [C] u64, depth histogram [13] u32, records [C, n_collect] of 16
 * bytes. */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../mini_mcmc_amd/csrc/mm_params.h"
#include "../../mini_mcmc_amd/csrc/mm_samplers.h"
#include "../../mini_mcmc_amd/csrc/mm_nuts.h"
#include "../../mini_mcmc_amd/csrc/mm_metric_host.h"

static long g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                                                               \
    do {                                                                               \
        ++g_checks;                                                                    \
        if (!(cond)) {                                                                 \
            if (++g_failed <= 20) {                                                    \
                std::printf("FAILED %s:%d %s -- ", __FILE__, __LINE__, #cond);         \
                std::printf(__VA_ARGS__);                                              \
                std::printf("\n");                                                     \
            }                                                                          \
        }                                                                              \
    } while (0)

static_assert(sizeof(mm_nuts_draw) == 16 && alignof(mm_nuts_draw) == 16, "the record is one 16-byte store");

template <class TT, class ST> struct nuts_result {
    std::vector<TT> samples, positions;
    std::vector<ST> adapt;
    std::vector<uint64_t> nlf;
    std::vector<int> depths;
    std::vector<mm_nuts_draw> rec; /* [C, n_collect]; empty under the empty policy */
    bool same_chain_state(const nuts_result &o) const
    {
        return samples.size() == o.samples.size() && std::memcmp(samples.data(), o.samples.data(), samples.size() * sizeof(TT)) == 0 &&
               std::memcmp(positions.data(), o.positions.data(), positions.size() * sizeof(TT)) == 0 &&
               std::memcmp(adapt.data(), o.adapt.data(), adapt.size() * sizeof(ST)) == 0 && nlf == o.nlf && depths == o.depths;
    }
    bool same_records(const nuts_result &o) const
    {
        return rec.size() == o.rec.size() && (rec.empty() || std::memcmp(rec.data(), o.rec.data(), rec.size() * sizeof(mm_nuts_draw)) == 0);
    }
};

template <class T> static T ulp_of(T v)
{
    const T a = std::fabs(v);
    return std::nextafter(a, (T)INFINITY) - a;
}

/* engine_host.cpp's nuts_chains with run()'s or run_progress' stepping, as the kernels take it (mm_nuts_run_body): init_chain,
 * then the transitions; `eps0 > 0`: the adaptation record starts at epsilon = epsilon_bar = eps0 (no search).  check: item (2)
 * on every transition (Rec = mm_draw_recorder only). */
template <class TT, class ST, class Tgt, class Met, class Rec>
nuts_result<TT, ST> run_nuts(const mm_tparams<TT> &P, const std::vector<double> &x0, size_t n, uint64_t seed, size_t n_collect, size_t n_discard,
                             bool progress, const Met &met, bool pairs, double eps0 = -1.0, bool check = false, int max_depth = 10)
{
    constexpr int D = Tgt::dim;
    using Red = mm_red_seq<TT, D>;
    const ST eps_tol = sizeof(ST) == 4 ? (ST)1.1920929e-7 : (ST)2.220446049250313e-16;
    const ST delta = (ST)0.8;
    unsigned n_pre, n_rec, write_initial;
    if (progress) {
        write_initial = 0;
        n_pre = (unsigned)n_discard;
        n_rec = (unsigned)n_collect;
    } else if (n_discard == 0) {
        write_initial = n_collect > 0;
        n_pre = 0;
        n_rec = (unsigned)(n_collect > 0 ? n_collect - 1 : 0);
    } else {
        write_initial = 0;
        n_pre = (unsigned)(n_discard - 1);
        n_rec = (unsigned)n_collect;
    }
    nuts_result<TT, ST> r;
    r.samples.assign(n * n_collect * D, TT(0));
    r.positions.assign(n * D, TT(0));
    r.adapt.assign(n * 4, ST(0));
    r.nlf.assign(n, 0);
    if (Rec::records)
        r.rec.assign(n * n_collect, mm_nuts_draw{0.f, 0.f, 0.f, 0u});
    std::vector<TT> vec(mm_nuts_stack<TT, ST, D>::vec_slots);
    std::vector<ST> al(mm_nuts_stack<TT, ST, D>::alpha_slots);
    std::vector<uint32_t> cn(mm_nuts_stack<TT, ST, D>::cnt_slots);
    mm_nuts_stack<TT, ST, D> stk;
    stk.vec = vec.data();
    stk.alpha = al.data();
    stk.cnt = cn.data();
    stk.stride = 1;
    for (size_t c = 0; c < n; ++c) {
        TT x[D];
        for (int i = 0; i < D; ++i)
            x[i] = (TT)x0[c * D + i];
        mm_nuts_adapt<ST> ad;
        ad.epsilon = eps0 > 0 ? (ST)eps0 : (ST)-1;
        ad.epsilon_bar = eps0 > 0 ? (ST)eps0 : (ST)1;
        ad.h_bar = (ST)0;
        ad.mu = (ST)std::log(10.0);
        mm_nuts_init_chain<TT, ST, Tgt, Red, Met>(P, x, &ad, eps_tol, seed, c, met);
        size_t row = 0;
        uint32_t m = 0;
        auto put = [&](const mm_nuts_draw *d) {
            for (int i = 0; i < D; ++i)
                r.samples[(c * n_collect + row) * D + i] = x[i];
            if (Rec::records)
                r.rec[c * n_collect + row] = *d;
            ++row;
        };
        if (write_initial) {
            const mm_nuts_draw d0 = mm_nuts_draw_none(ad.epsilon);
            put(&d0);
        }
        for (unsigned t = 0; t < n_pre + n_rec; ++t) {
            ++m;
            TT x_prev[D];
            for (int i = 0; i < D; ++i)
                x_prev[i] = x[i];
            const mm_nuts_adapt<ST> ad_prev = ad;
            mm_nuts_draw d{0.f, 0.f, 0.f, 0u};
            const mm_nuts_info inf =
                pairs ? mm_nuts_step_pairs<TT, ST, Tgt, Red, Met, Rec>(P, x, &ad, m, (uint32_t)n_discard, delta, max_depth, seed, c, stk, met, &d)
                      : mm_nuts_step<TT, ST, Tgt, Red, Met, Rec>(P, x, &ad, m, (uint32_t)n_discard, delta, max_depth, seed, c, stk, met, &d);
            r.nlf[c] += inf.n_leapfrog;
            r.depths.push_back(inf.depth);
            if (check && Rec::records) {
                CHECK((d.tree & 0xffffu) == inf.n_leapfrog && ((d.tree >> 16) & 15u) == (uint32_t)inf.depth, "chain %zu t %u: tree %08x, info %u leapfrogs depth %d",
                      c, t, d.tree, inf.n_leapfrog, inf.depth);
                CHECK(((d.tree >> 25) & 1u) == (inf.depth >= max_depth ? 1u : 0u) && (d.tree >> 31) == 0u, "chain %zu t %u: flag bits %08x", c, t, d.tree);
                CHECK((d.tree & ~(0xffffu | (15u << 16) | (1u << 24) | (1u << 25))) == 0u, "chain %zu t %u: stray bits %08x", c, t, d.tree);
                /* energy: the tree's own joint, begin_with()'s order of operations */
                TT mom0[D], grad[D];
                mm_nuts_momentum<D>(seed, c, m, mom0);
                const TT ulogp = Tgt::logp_grad(P, x_prev, grad);
                const ST joint = (ST)(double)(ulogp - Red::dot(mom0, mom0) * TT(0.5));
                const float want_e = (float)(-joint), want_eps = (float)ad_prev.epsilon;
                CHECK(std::memcmp(&want_e, &d.energy, 4) == 0, "chain %zu t %u: energy %a, want %a", c, t, (double)d.energy, (double)want_e);
                CHECK(std::memcmp(&want_eps, &d.step_size, 4) == 0, "chain %zu t %u: step size %a, want %a", c, t, (double)d.step_size, (double)want_eps);
                /* accept_stat: the transition again under the empty policy from the saved adaptation record */
                TT xr[D];
                for (int i = 0; i < D; ++i)
                    xr[i] = x_prev[i];
                mm_nuts_adapt<ST> adr = ad_prev;
                (void)mm_nuts_step<TT, ST, Tgt, Red, Met>(P, xr, &adr, m, (uint32_t)n_discard, delta, max_depth, seed, c, stk, met);
                const ST eta = ST(1) / (ST)(m + MM_NUTS_T0);
                const ST want_h = (ST(1) - eta) * ad_prev.h_bar + eta * (delta - (ST)d.accept_stat);
                const ST tol = ST(4) * ulp_of(adr.h_bar) + (sizeof(ST) == 8 ? eta * (ST)(0.5f * ulp_of(d.accept_stat)) : ST(0));
                CHECK(std::fabs(adr.h_bar - want_h) <= tol && d.accept_stat >= 0.f && d.accept_stat <= 1.f, "chain %zu t %u: h_bar %a, from the record %a (accept %a)", c, t,
                      (double)adr.h_bar, (double)want_h, (double)d.accept_stat);
                CHECK(std::memcmp(&adr, &ad, sizeof ad) == 0, "chain %zu t %u: the rerun's adaptation record differs", c, t);
            }
            if (t >= n_pre)
                put(&d);
        }
        for (int i = 0; i < D; ++i)
            r.positions[c * D + i] = x[i];
        r.adapt[4 * c] = ad.epsilon;
        r.adapt[4 * c + 1] = ad.epsilon_bar;
        r.adapt[4 * c + 2] = ad.h_bar;
        r.adapt[4 * c + 3] = ad.mu;
    }
    return r;
}

static std::vector<double> start(size_t n, int D)
{
    std::vector<double> x(n * D);
    for (size_t c = 0; c < n; ++c)
        for (int i = 0; i < D; ++i)
            x[c * D + i] = 0.05 * (double)((int)((c * 7 + (size_t)i * 13) % 17) - 8) + 0.01 * i;
    return x;
}
template <class T> static mm_tparams<T> params_of(int kind, const double *params)
{
    mm_tparams<T> P;
    std::memset(&P, 0, sizeof P);
    if (mm_fill_params<T>(kind, params, &P) != 0)
        std::abort();
    return P;
}
static const double kNoParams[8] = {0, 0, 0, 0, 0, 0, 0, 0};
static const double kUnitGauss2d[8] = {0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0, 0};
static const double kDiag[3] = {0.37, 2.9, 11.0};
/* a lower-triangular 3 x 3 factor with kDiag's diagonal and off-diagonal entries of its order */
static std::vector<double> general_factor()
{
    return {0.37, 0.0, 0.0, -0.8, 2.9, 0.0, 1.5, -2.25, 11.0};
}
template <class T> static mm_diag_metric<T, 3> diag_metric()
{
    mm_diag_metric<T, 3> m;
    for (int i = 0; i < 3; ++i) {
        m.s[i] = (T)kDiag[i];
        m.r[i] = T(1) / m.s[i];
    }
    return m;
}
template <class T> struct dense_factors {
    std::vector<T> l, li;
    dense_factors()
    {
        if (!mm_dense_prepare<T>(general_factor().data(), 3, l, li))
            std::abort();
    }
    mm_dense_metric<T, 3> metric() const { return mm_dense_metric<T, 3>(l.data(), li.data()); }
};

/* ---- (1), (2) ---- */
template <class TT, class ST, class Met> static void recorder_case(int mode, const char *metric, const Met &met)
{
    using Tgt = mm_target<TT, MM_ROSENBROCK_ND, 3>;
    const mm_tparams<TT> P = params_of<TT>(MM_ROSENBROCK_ND, kNoParams);
    const std::vector<double> x0 = start(8, 3);
    for (size_t nd : {(size_t)0, (size_t)10}) {
        const size_t nc = nd == 0 ? 31 : 21; /* 30 transitions either way */
        nuts_result<TT, ST> rec_walk[2];
        for (int pairs = 0; pairs < 2; ++pairs) {
            const auto off = run_nuts<TT, ST, Tgt, Met, mm_no_recorder>(P, x0, 8, 42, nc, nd, false, met, pairs != 0);
            const auto on = run_nuts<TT, ST, Tgt, Met, mm_draw_recorder>(P, x0, 8, 42, nc, nd, false, met, pairs != 0, -1.0, true);
            CHECK(off.same_chain_state(on), "mode %d %s n_discard %zu pairs %d: the recorder changed a chain", mode, metric, nd, pairs);
            CHECK(off.depths.size() == 8 * 30 && off.rec.empty() && on.rec.size() == 8 * nc, "mode %d %s: %zu transitions, %zu records", mode, metric,
                  off.depths.size(), on.rec.size());
            if (nd == 0)
                for (size_t c = 0; c < 8; ++c) {
                    const mm_nuts_draw &d = on.rec[c * nc];
                    CHECK(d.tree == (1u << 31) && d.accept_stat != d.accept_stat && d.energy != d.energy && d.step_size > 0.f,
                          "mode %d %s chain %zu: row 0 is not the no-transition record (%08x)", mode, metric, c, d.tree);
                }
            rec_walk[pairs] = on;
        }
        CHECK(rec_walk[0].same_records(rec_walk[1]), "mode %d %s n_discard %zu: the pair walk's records differ from the leaf walk's", mode, metric, nd);
        uint64_t lf = 0;
        for (uint64_t v : rec_walk[0].nlf)
            lf += v;
        CHECK(lf >= 8 * 30, "mode %d %s: %llu leapfrogs", mode, metric, (unsigned long long)lf); /* every transition takes at least one */
    }
    /* the depth-cap bit: max_depth 2 on the same chains */
    const auto capped = run_nuts<TT, ST, Tgt, Met, mm_draw_recorder>(P, x0, 8, 42, 21, 10, false, met, true, -1.0, true, 2);
    size_t n_cap = 0;
    for (const mm_nuts_draw &d : capped.rec)
        n_cap += (d.tree >> 25) & 1u;
    CHECK(n_cap > 0, "mode %d %s: no transition reached a depth cap of 2", mode, metric);
}
template <class TT, class ST> static void recorder_mode(int mode)
{
    recorder_case<TT, ST>(mode, "no metric", mm_no_metric());
    recorder_case<TT, ST>(mode, "diagonal", diag_metric<TT>());
    const dense_factors<TT> f;
    recorder_case<TT, ST>(mode, "dense", f.metric());
}

/* ---- (3) ---- */
template <class TT, class ST> static nuts_result<TT, ST> gauss_run(size_t n, size_t rows, double eps, uint64_t seed)
{
    using Tgt = mm_target<TT, MM_GAUSSIAN2D, 2>;
    const mm_tparams<TT> P = params_of<TT>(MM_GAUSSIAN2D, kUnitGauss2d);
    return run_nuts<TT, ST, Tgt, mm_no_metric, mm_draw_recorder>(P, start(n, 2), n, seed, rows, 0, false, mm_no_metric(), true, eps);
}
template <class TT, class ST> static void divergence(int mode)
{
    const size_t n = 96, rows = 20;
    const std::vector<double> x0 = start(n, 2);
    const auto forced = gauss_run<TT, ST>(n, rows, 64.0, 7), absent = gauss_run<TT, ST>(n, rows, 0.1, 7);
    bool all_div = true, none_div = true, rows_start = true, eps_kept = true;
    for (size_t c = 0; c < n; ++c)
        for (size_t t = 0; t < rows; ++t) {
            const mm_nuts_draw &f = forced.rec[c * rows + t], &a = absent.rec[c * rows + t];
            if (t == 0) {
                all_div = all_div && f.tree == (1u << 31);
                none_div = none_div && a.tree == (1u << 31);
            } else {
                all_div = all_div && f.tree == ((1u << 24) | (1u << 16) | 1u); /* divergent, depth 1, one leapfrog */
                none_div = none_div && ((a.tree >> 24) & 1u) == 0u && (a.tree & 0xffffu) >= 1u;
            }
            eps_kept = eps_kept && f.step_size == 64.f && a.step_size == 0.1f;
            for (int i = 0; i < 2; ++i)
                rows_start = rows_start && forced.samples[(c * rows + t) * 2 + i] == (TT)x0[c * 2 + i];
        }
    CHECK(all_div, "mode %d: epsilon 64 left a transition that is not (divergent, depth 1, one leapfrog)", mode);
    CHECK(rows_start, "mode %d: epsilon 64 moved a chain", mode);
    CHECK(none_div, "mode %d: epsilon 0.1 diverged", mode);
    CHECK(eps_kept, "mode %d: the step size changed", mode);
    bool moved = false;
    for (size_t j = 0; j < absent.positions.size(); ++j)
        moved = moved || absent.positions[j] != (TT)x0[j];
    CHECK(moved, "mode %d: epsilon 0.1 moved nothing", mode);
}

/* ---- the reference of the GPU tests ---- */
template <class T> static void write_raw(FILE *f, const std::vector<T> &v)
{
    if (!v.empty() && std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size())
        std::abort();
}
template <class TT, class ST> static int dump(const nuts_result<TT, ST> &r, const char *path)
{
    std::vector<double> adapt(r.adapt.begin(), r.adapt.end());
    std::vector<uint32_t> hist(MM_NUTS_JMAX + 1, 0);
    for (int d : r.depths)
        hist[d < MM_NUTS_JMAX ? d : MM_NUTS_JMAX] += 1;
    FILE *f = std::fopen(path, "wb");
    if (!f)
        return 2;
    write_raw(f, r.samples);
    write_raw(f, r.positions);
    write_raw(f, adapt);
    write_raw(f, r.nlf);
    write_raw(f, hist);
    write_raw(f, r.rec);
    return std::fclose(f) == 0 ? 0 : 2;
}
template <class TT, class ST>
static int dump_nuts(size_t n, size_t nc, size_t nd, bool progress, uint64_t seed, const std::string &metric, const char *path)
{
    using Tgt = mm_target<TT, MM_ROSENBROCK_ND, 3>;
    const mm_tparams<TT> P = params_of<TT>(MM_ROSENBROCK_ND, kNoParams);
    const std::vector<double> x0 = start(n, 3);
    if (metric == "none")
        return dump(run_nuts<TT, ST, Tgt, mm_no_metric, mm_draw_recorder>(P, x0, n, seed, nc, nd, progress, mm_no_metric(), true), path);
    if (metric == "diag")
        return dump(run_nuts<TT, ST, Tgt, mm_diag_metric<TT, 3>, mm_draw_recorder>(P, x0, n, seed, nc, nd, progress, diag_metric<TT>(), true), path);
    if (metric == "dense") {
        const dense_factors<TT> f;
        return dump(run_nuts<TT, ST, Tgt, mm_dense_metric<TT, 3>, mm_draw_recorder>(P, x0, n, seed, nc, nd, progress, f.metric(), true), path);
    }
    return 2;
}

int main(int argc, char **argv)
{
    if (argc > 1) {
        const std::string cmd = argv[1];
        if (cmd == "nuts" && argc == 10) {
            const int mode = std::atoi(argv[2]);
            const size_t n = std::strtoull(argv[3], nullptr, 10), nc = std::strtoull(argv[4], nullptr, 10), nd = std::strtoull(argv[5], nullptr, 10);
            const bool progress = std::atoi(argv[6]) != 0;
            const uint64_t seed = std::strtoull(argv[7], nullptr, 10);
            return mode == 0 ? dump_nuts<float, double>(n, nc, nd, progress, seed, argv[8], argv[9])
                             : mode == 1 ? dump_nuts<float, float>(n, nc, nd, progress, seed, argv[8], argv[9])
                                         : dump_nuts<double, double>(n, nc, nd, progress, seed, argv[8], argv[9]);
        }
        if (cmd == "gauss" && argc == 8) {
            const int mode = std::atoi(argv[2]);
            const size_t n = std::strtoull(argv[3], nullptr, 10), rows = std::strtoull(argv[4], nullptr, 10);
            const double eps = std::strtod(argv[5], nullptr);
            const uint64_t seed = std::strtoull(argv[6], nullptr, 10);
            return mode == 0 ? dump(gauss_run<float, double>(n, rows, eps, seed), argv[7])
                             : mode == 1 ? dump(gauss_run<float, float>(n, rows, eps, seed), argv[7]) : dump(gauss_run<double, double>(n, rows, eps, seed), argv[7]);
        }
        std::fprintf(stderr, "usage: see the comment at the top of draw_stats_twin.cpp\n");
        return 2;
    }
    recorder_mode<float, double>(0);
    recorder_mode<float, float>(1);
    recorder_mode<double, double>(2);
    divergence<float, double>(0);
    divergence<float, float>(1);
    divergence<double, double>(2);
    std::printf("checks %ld failed %ld\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
