/* metric_twin.cpp -- the diagonal metric of HMC and NUTS (csrc/mm_samplers.h: mm_diag_metric) on the host.
 *
 * A plain C++17 program around the very headers the kernels are compiled from, built with the flags of oracle/Makefile
 * (-ffp-contract=off), so what it computes is what the device computes, bit for bit.
 *
 * Without arguments it checks, and exits 0 only if every check held:
 *  (a) a metric of all ones gives the bits of no metric -- HMC over 64 transitions of 8 chains on RosenbrockND(3) in f32 and
 *      Gaussian2D in f64 (samples, final state, accept counts); NUTS over 30 transitions in each type mode (samples, final
 *      positions, adaptation records, leapfrog counts, depths), walked leaf by leaf and in pairs;
 *  (b) the power-of-two identity: for logp = -1/2 sum (x_i c_i)^2, g_i = -(x_i c_i) c_i, with c_i = 2^-k_i and metric
 *      s_i = 2^k_i every product and rounding commutes with the scaling, so the metric run from x0 = s * y0 equals s * (the
 *      run without a metric of the same functor with c_i = 1 from y0) bit for bit -- samples, accept counts, adaptation
 *      records, leapfrog counts, depths; k_i in -6 .. 6, dimensions 1, 3, 9, 32, HMC with L in {0, 1, 7} in f32 and f64, NUTS
 *      in the three modes.
 * With arguments it is the reference of the GPU tests and of the float64 restatement (tests/metric_common.py):
 *   metric_twin hmc <f32|f64> <rosen3|gauss2d> <chains> <n_collect> <n_discard> <eps> <L> <seed> <out file> <print 0|1> [s_0 ..]
 *   metric_twin nuts <mode> <chains> <n_collect> <n_discard> <seed> <out file> [s_0 s_1 s_2]          (RosenbrockND(3))
 * from the fixed start x0[c][i] = 0.05 * ((7 c + 13 i) mod 17 - 8) + 0.01 i; no scales = no metric.  The out file holds, raw:
 * HMC samples [C, n_collect, D], state [C, D] (element type), accept counts [C] u64; NUTS samples, positions (tensor type),
 * adaptation records [C, 4] f64, leapfrog counts [C] u64, depth histogram [13] u32.  print = 1: every transition's momentum
 * noise, ln u, state and accept decision of every chain as hexadecimal floats on stdout. */
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

/* logp = -1/2 sum (x_i c_i)^2 with c = P.mat[0 .. D) */
template <class T, int Dm> struct quad_target {
    static constexpr int dim = Dm;
    static T logp(const mm_tparams<T> &P, const T *x)
    {
        T s = 0;
        for (int i = 0; i < Dm; ++i) {
            const T t = x[i] * P.mat[i];
            s = mm_fma(t, t, s);
        }
        return T(-0.5) * s;
    }
    static T logp_grad(const mm_tparams<T> &P, const T *x, T *g)
    {
        T s = 0;
        for (int i = 0; i < Dm; ++i) {
            const T t = x[i] * P.mat[i];
            s = mm_fma(t, t, s);
            g[i] = -t * P.mat[i];
        }
        return T(-0.5) * s;
    }
};

template <class T> struct hmc_result {
    std::vector<T> samples, state;
    std::vector<uint64_t> accept;
    bool operator==(const hmc_result &o) const
    {
        return samples.size() == o.samples.size() && std::memcmp(samples.data(), o.samples.data(), samples.size() * sizeof(T)) == 0 &&
               std::memcmp(state.data(), o.state.data(), state.size() * sizeof(T)) == 0 && accept == o.accept;
    }
};

/* engine_host.cpp's run_chains for HMC, with a metric; print: the noise and the states as text */
template <class T, class Tgt, class Met>
hmc_result<T> run_hmc(const mm_tparams<T> &P, T eps, int L, const std::vector<T> &x0, size_t n_chains, uint64_t seed, size_t n_collect,
                      size_t n_discard, const Met &met, bool print = false)
{
    constexpr int D = Tgt::dim;
    hmc_result<T> r;
    r.samples.assign(n_chains * n_collect * D, T(0));
    r.state = x0;
    r.accept.assign(n_chains, 0);
    for (size_t c = 0; c < n_chains; ++c) {
        T x[D], g[D], lp;
        for (int i = 0; i < D; ++i)
            x[i] = x0[c * D + i];
        lp = Tgt::logp_grad(P, x, g);
        uint32_t it = 0;
        for (size_t t = 0; t < n_discard + n_collect; ++t, ++it) {
            if (print) {
                T p[D], u;
                mm_draw_noise<D>(seed, c, it, p, &u);
                std::printf("noise %zu %zu", c, t);
                for (int i = 0; i < D; ++i)
                    std::printf(" %a", (double)p[i]);
                std::printf(" %a\n", (double)mm_ln_accept(u, mm_icdf_global()));
            }
            const int acc = mm_hmc_step<T, Tgt, Met>(P, eps, L, x, &lp, g, seed, c, it, met);
            r.accept[c] += (uint64_t)acc;
            if (print) {
                std::printf("state %zu %zu", c, t);
                for (int i = 0; i < D; ++i)
                    std::printf(" %a", (double)x[i]);
                std::printf(" %d\n", acc);
            }
            if (t >= n_discard)
                for (int i = 0; i < D; ++i)
                    r.samples[(c * n_collect + (t - n_discard)) * D + i] = x[i];
        }
        for (int i = 0; i < D; ++i)
            r.state[c * D + i] = x[i];
    }
    return r;
}

template <class TT, class ST> struct nuts_result {
    std::vector<TT> samples, positions;
    std::vector<ST> adapt;
    std::vector<uint64_t> nlf;
    std::vector<int> depths; /* of every transition of every chain, in order */
    bool operator==(const nuts_result &o) const
    {
        return samples.size() == o.samples.size() && std::memcmp(samples.data(), o.samples.data(), samples.size() * sizeof(TT)) == 0 &&
               std::memcmp(positions.data(), o.positions.data(), positions.size() * sizeof(TT)) == 0 &&
               std::memcmp(adapt.data(), o.adapt.data(), adapt.size() * sizeof(ST)) == 0 && nlf == o.nlf && depths == o.depths;
    }
};

/* engine_host.cpp's nuts_chains with run()'s stepping (N - 1 transitions), fresh adaptation records, with a metric */
template <class TT, class ST, class Tgt, class Met>
nuts_result<TT, ST> run_nuts(const mm_tparams<TT> &P, const std::vector<double> &x0, size_t n, uint64_t seed, size_t n_collect, size_t n_discard,
                             const Met &met, bool pairs)
{
    constexpr int D = Tgt::dim;
    using Red = mm_red_seq<TT, D>;
    const ST eps_tol = sizeof(ST) == 4 ? (ST)1.1920929e-7 : (ST)2.220446049250313e-16;
    unsigned n_pre, n_rec, write_initial;
    if (n_discard == 0) {
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
        ad.epsilon = (ST)-1;
        ad.epsilon_bar = (ST)1;
        ad.h_bar = (ST)0;
        ad.mu = (ST)std::log(10.0);
        mm_nuts_init_chain<TT, ST, Tgt, Red, Met>(P, x, &ad, eps_tol, seed, c, met);
        size_t row = 0;
        uint32_t m = 0;
        auto rec = [&]() {
            for (int i = 0; i < D; ++i)
                r.samples[(c * n_collect + row) * D + i] = x[i];
            ++row;
        };
        if (write_initial)
            rec();
        for (unsigned t = 0; t < n_pre + n_rec; ++t) {
            ++m;
            const mm_nuts_info inf =
                pairs ? mm_nuts_step_pairs<TT, ST, Tgt, Red, Met>(P, x, &ad, m, (uint32_t)n_discard, (ST)0.8, 10, seed, c, stk, met)
                      : mm_nuts_step<TT, ST, Tgt, Red, Met>(P, x, &ad, m, (uint32_t)n_discard, (ST)0.8, 10, seed, c, stk, met);
            r.nlf[c] += inf.n_leapfrog;
            r.depths.push_back(inf.depth);
            if (t >= n_pre)
                rec();
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
template <class T> static std::vector<T> as(const std::vector<double> &v)
{
    std::vector<T> o(v.size());
    for (size_t i = 0; i < v.size(); ++i)
        o[i] = (T)v[i];
    return o;
}
template <class T, int D> static mm_diag_metric<T, D> metric_of(const double *s)
{
    mm_diag_metric<T, D> m;
    for (int i = 0; i < D; ++i) {
        m.s[i] = (T)s[i];
        m.r[i] = T(1) / m.s[i];
    }
    return m;
}
template <class T> static mm_tparams<T> params_of(int kind, const double *params)
{
    mm_tparams<T> P;
    std::memset(&P, 0, sizeof P);
    if (mm_fill_params<T>(kind, params, &P) != 0)
        std::abort();
    return P;
}
static const double kGauss2d[8] = {0.0, 1.0, 4.0, 2.0, 2.0, 3.0, 0, 0};

/* ---- (a): ones = none ---- */
template <class T, class Tgt> static void ones_hmc(const char *what, int kind, const double *params)
{
    constexpr int D = Tgt::dim;
    const mm_tparams<T> P = params_of<T>(kind, params);
    const std::vector<T> x0 = as<T>(start(8, D));
    double ones[D];
    for (int i = 0; i < D; ++i)
        ones[i] = 1.0;
    for (int L : {0, 1, 7}) {
        const auto a = run_hmc<T, Tgt>(P, (T)0.05, L, x0, 8, 42, 40, 24, mm_no_metric());
        const auto b = run_hmc<T, Tgt>(P, (T)0.05, L, x0, 8, 42, 40, 24, metric_of<T, D>(ones));
        CHECK(a == b, "HMC %s L %d: a metric of ones differs from no metric", what, L);
        uint64_t acc = 0;
        for (uint64_t v : a.accept)
            acc += v;
        CHECK(L == 0 || (acc > 0 && std::memcmp(a.state.data(), x0.data(), x0.size() * sizeof(T)) != 0), "HMC %s L %d: nothing moved", what, L);
    }
}
template <class TT, class ST> static void ones_nuts(int mode)
{
    using Tgt = mm_target<TT, MM_ROSENBROCK_ND, 3>;
    const mm_tparams<TT> P = params_of<TT>(MM_ROSENBROCK_ND, kGauss2d);
    const std::vector<double> x0 = start(8, 3);
    const double ones[3] = {1.0, 1.0, 1.0};
    const auto a = run_nuts<TT, ST, Tgt>(P, x0, 8, 42, 20, 11, mm_no_metric(), false);
    for (int pairs = 0; pairs < 2; ++pairs) {
        const auto b = run_nuts<TT, ST, Tgt>(P, x0, 8, 42, 20, 11, metric_of<TT, 3>(ones), pairs != 0);
        CHECK(a == b, "NUTS mode %d pairs %d: a metric of ones differs from no metric", mode, pairs);
    }
    CHECK(a.depths.size() == 8 * 30, "NUTS mode %d: %zu transitions", mode, a.depths.size());
    /* a general metric: leaf by leaf and in pairs are the same walk */
    const double gen[3] = {0.37, 2.9, 11.0};
    CHECK((run_nuts<TT, ST, Tgt>(P, x0, 8, 42, 20, 11, metric_of<TT, 3>(gen), false) == run_nuts<TT, ST, Tgt>(P, x0, 8, 42, 20, 11, metric_of<TT, 3>(gen), true)),
          "NUTS mode %d: pairs differ from leaves under a general metric", mode);
    CHECK(!(run_nuts<TT, ST, Tgt>(P, x0, 8, 42, 20, 11, metric_of<TT, 3>(gen), false) == a), "NUTS mode %d: a general metric changed nothing", mode);
}

/* ---- (b): the power-of-two identity ---- */
template <int D> static void pow2_scales(double *s, double *c, double *one)
{
    for (int i = 0; i < D; ++i) {
        const int k = (i * 5 + 3) % 13 - 6; /* -6 .. 6 */
        s[i] = std::ldexp(1.0, k);
        c[i] = std::ldexp(1.0, -k);
        one[i] = 1.0;
    }
}
template <class T, int D> static void pow2_hmc(const char *ty)
{
    using Tgt = quad_target<T, D>;
    double s[D], c[D], one[D];
    pow2_scales<D>(s, c, one);
    const std::vector<T> cs = as<T>(std::vector<double>(c, c + D)), c1 = as<T>(std::vector<double>(one, one + D));
    mm_tparams<T> Ps, P1;
    std::memset(&Ps, 0, sizeof Ps);
    std::memset(&P1, 0, sizeof P1);
    Ps.mat = cs.data();
    P1.mat = c1.data();
    const size_t n = 8;
    std::vector<double> y0 = start(n, D), xs0(n * D);
    for (size_t j = 0; j < n * D; ++j) {
        y0[j] *= 8.0; /* of the order of the unit scale */
        xs0[j] = y0[j] * s[j % D];
    }
    for (int L : {0, 1, 7}) {
        const auto a = run_hmc<T, Tgt>(Ps, (T)0.3, L, as<T>(xs0), n, 7, 14, 6, metric_of<T, D>(s));
        const auto b = run_hmc<T, Tgt>(P1, (T)0.3, L, as<T>(y0), n, 7, 14, 6, mm_no_metric());
        bool same = a.accept == b.accept;
        for (size_t j = 0; j < a.samples.size() && same; ++j) {
            const T want = b.samples[j] * (T)s[j % D];
            same = std::memcmp(&want, &a.samples[j], sizeof(T)) == 0;
        }
        for (size_t j = 0; j < a.state.size() && same; ++j) {
            const T want = b.state[j] * (T)s[j % D];
            same = std::memcmp(&want, &a.state[j], sizeof(T)) == 0;
        }
        CHECK(same, "HMC %s dim %d L %d: the power-of-two identity", ty, D, L);
        uint64_t acc = 0;
        for (uint64_t v : a.accept)
            acc += v;
        CHECK(L == 0 || acc > 0, "HMC %s dim %d L %d: no accept", ty, D, L);
    }
}
template <class TT, class ST, int D> static void pow2_nuts(int mode)
{
    using Tgt = quad_target<TT, D>;
    double s[D], c[D], one[D];
    pow2_scales<D>(s, c, one);
    const std::vector<TT> cs = as<TT>(std::vector<double>(c, c + D)), c1 = as<TT>(std::vector<double>(one, one + D));
    mm_tparams<TT> Ps, P1;
    std::memset(&Ps, 0, sizeof Ps);
    std::memset(&P1, 0, sizeof P1);
    Ps.mat = cs.data();
    P1.mat = c1.data();
    const size_t n = 4;
    std::vector<double> y0 = start(n, D), xs0(n * D);
    for (size_t j = 0; j < n * D; ++j) {
        y0[j] = (double)(TT)(y0[j] * 8.0); /* exactly representable in the tensor type, so that x0 = s * y0 is exact there too */
        xs0[j] = y0[j] * s[j % D];
    }
    for (int pairs = 0; pairs < 2; ++pairs) {
        const auto a = run_nuts<TT, ST, Tgt>(Ps, xs0, n, 7, 10, 6, metric_of<TT, D>(s), pairs != 0);
        const auto b = run_nuts<TT, ST, Tgt>(P1, y0, n, 7, 10, 6, mm_no_metric(), pairs != 0);
        bool same = a.nlf == b.nlf && a.depths == b.depths && std::memcmp(a.adapt.data(), b.adapt.data(), a.adapt.size() * sizeof(ST)) == 0;
        for (size_t j = 0; j < a.samples.size() && same; ++j) {
            const TT want = b.samples[j] * (TT)s[j % D];
            same = std::memcmp(&want, &a.samples[j], sizeof(TT)) == 0;
        }
        for (size_t j = 0; j < a.positions.size() && same; ++j) {
            const TT want = b.positions[j] * (TT)s[j % D];
            same = std::memcmp(&want, &a.positions[j], sizeof(TT)) == 0;
        }
        CHECK(same, "NUTS mode %d dim %d pairs %d: the power-of-two identity", mode, D, pairs);
        uint64_t lf = 0;
        for (uint64_t v : a.nlf)
            lf += v;
        CHECK(lf >= n * 15, "NUTS mode %d dim %d: %llu leapfrogs", mode, D, (unsigned long long)lf);
    }
}
template <int D> static void pow2_dim()
{
    pow2_hmc<float, D>("f32");
    pow2_hmc<double, D>("f64");
    pow2_nuts<float, double, D>(0);
    pow2_nuts<float, float, D>(1);
    pow2_nuts<double, double, D>(2);
}

/* ---- the reference of the GPU tests ---- */
template <class T> static void write_raw(FILE *f, const std::vector<T> &v)
{
    if (!v.empty() && std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size())
        std::abort();
}
template <class T, class Tgt>
static int dump_hmc(int kind, const double *params, size_t n, size_t nc, size_t nd, double eps, int L, uint64_t seed, const char *path, bool print,
                    const std::vector<double> &s)
{
    constexpr int D = Tgt::dim;
    if (!s.empty() && s.size() != (size_t)D)
        return 2;
    const mm_tparams<T> P = params_of<T>(kind, params);
    const std::vector<T> x0 = as<T>(start(n, D));
    const hmc_result<T> r = s.empty() ? run_hmc<T, Tgt>(P, (T)eps, L, x0, n, seed, nc, nd, mm_no_metric(), print)
                                      : run_hmc<T, Tgt>(P, (T)eps, L, x0, n, seed, nc, nd, metric_of<T, D>(s.data()), print);
    FILE *f = std::fopen(path, "wb");
    if (!f)
        return 2;
    write_raw(f, r.samples);
    write_raw(f, r.state);
    write_raw(f, r.accept);
    return std::fclose(f) == 0 ? 0 : 2;
}
template <class TT, class ST>
static int dump_nuts(size_t n, size_t nc, size_t nd, uint64_t seed, const char *path, const std::vector<double> &s)
{
    using Tgt = mm_target<TT, MM_ROSENBROCK_ND, 3>;
    if (!s.empty() && s.size() != 3)
        return 2;
    const mm_tparams<TT> P = params_of<TT>(MM_ROSENBROCK_ND, kGauss2d);
    const std::vector<double> x0 = start(n, 3);
    const nuts_result<TT, ST> r = s.empty() ? run_nuts<TT, ST, Tgt>(P, x0, n, seed, nc, nd, mm_no_metric(), true)
                                            : run_nuts<TT, ST, Tgt>(P, x0, n, seed, nc, nd, metric_of<TT, 3>(s.data()), true);
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
    return std::fclose(f) == 0 ? 0 : 2;
}

int main(int argc, char **argv)
{
    if (argc > 1) {
        const std::string cmd = argv[1];
        std::vector<double> s;
        if (cmd == "hmc" && argc >= 12) {
            const bool f64 = std::string(argv[2]) == "f64", rosen = std::string(argv[3]) == "rosen3";
            const size_t n = std::strtoull(argv[4], nullptr, 10), nc = std::strtoull(argv[5], nullptr, 10), nd = std::strtoull(argv[6], nullptr, 10);
            const double eps = std::strtod(argv[7], nullptr);
            const int L = std::atoi(argv[8]);
            const uint64_t seed = std::strtoull(argv[9], nullptr, 10);
            const bool print = std::atoi(argv[11]) != 0;
            for (int i = 12; i < argc; ++i)
                s.push_back(std::strtod(argv[i], nullptr));
            if (rosen)
                return f64 ? dump_hmc<double, mm_target<double, MM_ROSENBROCK_ND, 3>>(MM_ROSENBROCK_ND, kGauss2d, n, nc, nd, eps, L, seed, argv[10], print, s)
                           : dump_hmc<float, mm_target<float, MM_ROSENBROCK_ND, 3>>(MM_ROSENBROCK_ND, kGauss2d, n, nc, nd, eps, L, seed, argv[10], print, s);
            return f64 ? dump_hmc<double, mm_target<double, MM_GAUSSIAN2D, 2>>(MM_GAUSSIAN2D, kGauss2d, n, nc, nd, eps, L, seed, argv[10], print, s)
                       : dump_hmc<float, mm_target<float, MM_GAUSSIAN2D, 2>>(MM_GAUSSIAN2D, kGauss2d, n, nc, nd, eps, L, seed, argv[10], print, s);
        }
        if (cmd == "nuts" && argc >= 8) {
            const int mode = std::atoi(argv[2]);
            const size_t n = std::strtoull(argv[3], nullptr, 10), nc = std::strtoull(argv[4], nullptr, 10), nd = std::strtoull(argv[5], nullptr, 10);
            const uint64_t seed = std::strtoull(argv[6], nullptr, 10);
            for (int i = 8; i < argc; ++i)
                s.push_back(std::strtod(argv[i], nullptr));
            return mode == 0 ? dump_nuts<float, double>(n, nc, nd, seed, argv[7], s)
                             : mode == 1 ? dump_nuts<float, float>(n, nc, nd, seed, argv[7], s) : dump_nuts<double, double>(n, nc, nd, seed, argv[7], s);
        }
        std::fprintf(stderr, "usage: see the comment at the top of metric_twin.cpp\n");
        return 2;
    }
    ones_hmc<float, mm_target<float, MM_ROSENBROCK_ND, 3>>("RosenbrockND(3) f32", MM_ROSENBROCK_ND, kGauss2d);
    ones_hmc<double, mm_target<double, MM_GAUSSIAN2D, 2>>("Gaussian2D f64", MM_GAUSSIAN2D, kGauss2d);
    ones_nuts<float, double>(0);
    ones_nuts<float, float>(1);
    ones_nuts<double, double>(2);
    pow2_dim<1>();
    pow2_dim<3>();
    pow2_dim<9>();
    pow2_dim<32>();
    std::printf("checks %ld failed %ld\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
