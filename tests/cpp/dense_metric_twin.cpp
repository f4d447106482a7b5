/* dense_metric_twin.cpp -- the dense metric of HMC and NUTS (csrc/mm_samplers.h: mm_dense_metric) on the host.
 *
 * A plain C++17 program around the very headers the kernels are compiled from, built with the flags of oracle/Makefile
 * (-ffp-contract=off), so what it computes is what the device computes, bit for bit.  The factors come from
 * csrc/mm_metric_host.h, which the library's setters use too.  The runners (run_hmc, run_nuts, start, ...) are those of the
 * diagonal metric's twin, metric_twin.cpp, included below with its main() renamed: they take the metric as a type.
 *
 * Without arguments it checks, at dims 2 (Gaussian2D), 3, 9 and 32 (RosenbrockND), HMC in f32 and f64 with L in {1, 7} and NUTS
 * in the three type modes walked leaf by leaf and in pairs, and exits 0 only if every check held:
 *  (a) an identity factor gives the bits of no metric;
 *  (b) a factor diag(s), every s_i a power of two, gives the bits of the diagonal metric s;
 *  (c) under a general factor NUTS's pairs equal its leaves, and the run differs from the one without a metric.
 * With arguments it is the reference of the GPU tests and of the float64 restatement (tests/dense_metric_common.py):
 *   dense_metric_twin hmc <f32|f64> <dim> <chains> <n_collect> <n_discard> <eps> <L> <seed> <out file> <print 0|1> <factor file>
 *   dense_metric_twin nuts <mode> <dim> <chains> <n_collect> <n_discard> <seed> <out file> <factor file>
 * dim 2 is Gaussian2D, dims 3, 9, 32 RosenbrockND; the factor file holds dim x dim float64, row-major; the start and the out
 * file are metric_twin.cpp's.  The checks (a) - (c) cannot see L and L^T swapped in the kick (an identity or diagonal factor is
 * its own transpose); the float64 restatement of tests/test_dense_metric_host.py and the device comparison under
 * general_factor can, and do. */
#define main metric_twin_main
#include "metric_twin.cpp"
#undef main

#include "../../mini_mcmc_amd/csrc/mm_metric_host.h"

/* the two packed factors, each in a heap block of exactly D (D + 1) / 2 elements, and the metric that points at them */
template <class T, int D> struct dense_factors {
    std::vector<T> l, li;
    explicit dense_factors(const std::vector<double> &chol)
    {
        if (chol.size() != (size_t)D * D || !mm_dense_prepare<T>(chol.data(), (size_t)D, l, li))
            std::abort();
        l.shrink_to_fit();
        li.shrink_to_fit();
    }
    mm_dense_metric<T, D> metric() const { return mm_dense_metric<T, D>(l.data(), li.data()); }
};

template <int D> static std::vector<double> identity_factor()
{
    std::vector<double> c((size_t)D * D, 0.0);
    for (int i = 0; i < D; ++i)
        c[(size_t)i * D + i] = 1.0;
    return c;
}
template <int D> static std::vector<double> pow2_factor(double *s)
{
    std::vector<double> c((size_t)D * D, 0.0);
    for (int i = 0; i < D; ++i) {
        s[i] = std::ldexp(1.0, (i * 5 + 3) % 7 - 3); /* 2^-3 .. 2^3 */
        c[(size_t)i * D + i] = s[i];
    }
    return c;
}
/* large off-diagonal entries against a diagonal of 0.5 .. 1: nothing near the identity */
template <int D> static std::vector<double> general_factor()
{
    std::vector<double> c((size_t)D * D, 0.0);
    for (int i = 0; i < D; ++i) {
        c[(size_t)i * D + i] = 0.5 + 0.25 * (i % 3);
        for (int j = 0; j < i; ++j)
            c[(size_t)i * D + j] = 0.6 * (double)((i * 7 + j * 3) % 5 - 2) / std::sqrt((double)D);
    }
    return c;
}

template <int D> struct target_of {
    static constexpr int kind = D == 2 ? MM_GAUSSIAN2D : MM_ROSENBROCK_ND;
    template <class T> using type = mm_target<T, kind, D>;
};

template <class T, int D> static void check_hmc(const char *ty)
{
    using Tgt = typename target_of<D>::template type<T>;
    const mm_tparams<T> P = params_of<T>(target_of<D>::kind, kGauss2d);
    const size_t n = 6;
    const std::vector<T> x0 = as<T>(start(n, D));
    const T eps = (T)(D == 2 ? 0.3 : 0.01);
    double s[D];
    const dense_factors<T, D> ident(identity_factor<D>()), p2(pow2_factor<D>(s)), gen(general_factor<D>());
    for (int L : {1, 7}) {
        const auto none = run_hmc<T, Tgt>(P, eps, L, x0, n, 42, 20, 8, mm_no_metric());
        CHECK((run_hmc<T, Tgt>(P, eps, L, x0, n, 42, 20, 8, ident.metric()) == none), "HMC %s dim %d L %d: an identity factor differs from no metric", ty,
              D, L);
        CHECK((run_hmc<T, Tgt>(P, eps, L, x0, n, 42, 20, 8, p2.metric()) == run_hmc<T, Tgt>(P, eps, L, x0, n, 42, 20, 8, metric_of<T, D>(s))),
              "HMC %s dim %d L %d: a power-of-two diagonal factor differs from the diagonal metric", ty, D, L);
        if (L == 7)
            CHECK(!(run_hmc<T, Tgt>(P, eps, L, x0, n, 42, 20, 8, gen.metric()) == none), "HMC %s dim %d: a general factor changed nothing", ty, D);
    }
}
template <class TT, class ST, int D> static void check_nuts(int mode)
{
    using Tgt = typename target_of<D>::template type<TT>;
    const mm_tparams<TT> P = params_of<TT>(target_of<D>::kind, kGauss2d);
    const size_t n = 4, nc = 8, nd = 6;
    const std::vector<double> x0 = start(n, D);
    double s[D];
    const dense_factors<TT, D> ident(identity_factor<D>()), p2(pow2_factor<D>(s)), gen(general_factor<D>());
    const auto none = run_nuts<TT, ST, Tgt>(P, x0, n, 42, nc, nd, mm_no_metric(), false);
    for (int pairs = 0; pairs < 2; ++pairs) {
        CHECK((run_nuts<TT, ST, Tgt>(P, x0, n, 42, nc, nd, ident.metric(), pairs != 0) == none),
              "NUTS mode %d dim %d pairs %d: an identity factor differs from no metric", mode, D, pairs);
        CHECK((run_nuts<TT, ST, Tgt>(P, x0, n, 42, nc, nd, p2.metric(), pairs != 0) == run_nuts<TT, ST, Tgt>(P, x0, n, 42, nc, nd, metric_of<TT, D>(s), pairs != 0)),
              "NUTS mode %d dim %d pairs %d: a power-of-two diagonal factor differs from the diagonal metric", mode, D, pairs);
    }
    const auto g = run_nuts<TT, ST, Tgt>(P, x0, n, 42, nc, nd, gen.metric(), false);
    CHECK((run_nuts<TT, ST, Tgt>(P, x0, n, 42, nc, nd, gen.metric(), true) == g), "NUTS mode %d dim %d: pairs differ from leaves under a general factor", mode, D);
    CHECK(!(g == none), "NUTS mode %d dim %d: a general factor changed nothing", mode, D);
}
template <int D> static void check_dim()
{
    check_hmc<float, D>("f32");
    check_hmc<double, D>("f64");
    check_nuts<float, double, D>(0);
    check_nuts<float, float, D>(1);
    check_nuts<double, double, D>(2);
}

/* ---- the reference of the GPU tests ---- */
static std::vector<double> read_factor(const char *path, int D)
{
    std::vector<double> c((size_t)D * D);
    FILE *f = std::fopen(path, "rb");
    if (!f || std::fread(c.data(), sizeof(double), c.size(), f) != c.size())
        std::abort();
    std::fclose(f);
    return c;
}
template <class T, int D>
static int dense_dump_hmc(size_t n, size_t nc, size_t nd, double eps, int L, uint64_t seed, const char *path, bool print, const char *factor)
{
    using Tgt = typename target_of<D>::template type<T>;
    const mm_tparams<T> P = params_of<T>(target_of<D>::kind, kGauss2d);
    const dense_factors<T, D> fac(read_factor(factor, D));
    const hmc_result<T> r = run_hmc<T, Tgt>(P, (T)eps, L, as<T>(start(n, D)), n, seed, nc, nd, fac.metric(), print);
    FILE *f = std::fopen(path, "wb");
    if (!f)
        return 2;
    write_raw(f, r.samples);
    write_raw(f, r.state);
    write_raw(f, r.accept);
    return std::fclose(f) == 0 ? 0 : 2;
}
template <class TT, class ST, int D> static int dense_dump_nuts(size_t n, size_t nc, size_t nd, uint64_t seed, const char *path, const char *factor)
{
    using Tgt = typename target_of<D>::template type<TT>;
    const mm_tparams<TT> P = params_of<TT>(target_of<D>::kind, kGauss2d);
    const dense_factors<TT, D> fac(read_factor(factor, D));
    const nuts_result<TT, ST> r = run_nuts<TT, ST, Tgt>(P, start(n, D), n, seed, nc, nd, fac.metric(), true);
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
template <int D> static int dense_cmd(int argc, char **argv)
{
    const std::string cmd = argv[1];
    if (cmd == "hmc" && argc == 13) {
        const bool f64 = std::string(argv[2]) == "f64";
        const size_t n = std::strtoull(argv[4], nullptr, 10), nc = std::strtoull(argv[5], nullptr, 10), nd = std::strtoull(argv[6], nullptr, 10);
        const double eps = std::strtod(argv[7], nullptr);
        const int L = std::atoi(argv[8]);
        const uint64_t seed = std::strtoull(argv[9], nullptr, 10);
        const bool print = std::atoi(argv[11]) != 0;
        return f64 ? dense_dump_hmc<double, D>(n, nc, nd, eps, L, seed, argv[10], print, argv[12])
                   : dense_dump_hmc<float, D>(n, nc, nd, eps, L, seed, argv[10], print, argv[12]);
    }
    if (cmd == "nuts" && argc == 10) {
        const int mode = std::atoi(argv[2]);
        const size_t n = std::strtoull(argv[4], nullptr, 10), nc = std::strtoull(argv[5], nullptr, 10), nd = std::strtoull(argv[6], nullptr, 10);
        const uint64_t seed = std::strtoull(argv[7], nullptr, 10);
        return mode == 0   ? dense_dump_nuts<float, double, D>(n, nc, nd, seed, argv[8], argv[9])
               : mode == 1 ? dense_dump_nuts<float, float, D>(n, nc, nd, seed, argv[8], argv[9])
                           : dense_dump_nuts<double, double, D>(n, nc, nd, seed, argv[8], argv[9]);
    }
    return 2;
}

int main(int argc, char **argv)
{
    if (argc > 3) {
        const int dim = std::atoi(argv[3]);
        const int rc = dim == 2 ? dense_cmd<2>(argc, argv) : dim == 3 ? dense_cmd<3>(argc, argv) : dim == 9 ? dense_cmd<9>(argc, argv)
                                                                   : dim == 32 ? dense_cmd<32>(argc, argv) : 2;
        if (rc == 2)
            std::fprintf(stderr, "usage: see the comment at the top of dense_metric_twin.cpp\n");
        return rc;
    }
    if (argc > 1)
        return 2;
    check_dim<2>();
    check_dim<3>();
    check_dim<9>();
    check_dim<32>();
    std::printf("checks %ld failed %ld\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
