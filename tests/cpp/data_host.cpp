/* Host evaluation of the models that carry data (tests/data_common.py, tests/test_data_target_host.py, tests/test_data_target_gpu.py).
 *
 * Plain C++ with the flags of the host twin (-ffp-contract=off): the same functor code the device runs (csrc/mm_data.h,
 * csrc/mm_autodiff.h), so the file this program writes is what mmcmc_logp_grad_batch must return bit for bit.  The models live
 * in data_cases/ (one file per spelling); the GPU tests register those very files.
 *
 * usage: data_host <out.bin> <data.bin>
 * <data.bin>: the bound arrays as float64, linreg3's 28 values, then logit9's 50; converted to the element type once, the way a
 * create path does.  The arrays are allocated with exactly data_len elements, so a row helper that reads one element too
 * many is an AddressSanitizer report.
 * Output, per case and element type (the layout of tests/cpp/autodiff_host.cpp):
 *     x[n][dim]  value_ad[n]  value_plain[n]  grad_ad[n][dim]  and, where a hand-written gradient exists,  value_hand[n]  grad_hand[n][dim]
 * and one index line:  <case> <f32|f64> <dim> <n> <byte offset> <0|1: hand-written gradient present>
 */
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../mini_mcmc_amd/csrc/mm_data.h"

namespace linreg3 {
#include "data_cases/linreg3_logp.inc"
#include "data_cases/linreg3_hand.inc"
} // namespace linreg3
namespace logit9 {
#include "data_cases/logit9_logp.inc"
#include "data_cases/logit9_hand.inc"
} // namespace logit9
namespace softplus {
#include "data_cases/softplus.inc"
}
namespace softplus_composed {
#include "data_cases/softplus_composed.inc"
}
namespace sigmoid {
#include "data_cases/sigmoid.inc"
}

struct no_hand {};
template <class A, class B> struct is_same_type { static constexpr bool value = false; };
template <class A> struct is_same_type<A, A> { static constexpr bool value = true; };
template <class T> using none = no_hand;

constexpr int N_POINTS = 257;

/* the grid of autodiff_host.cpp, |x| <= 2, every coordinate exact in f32: 129 multiples of 1/8, then multiples of 1/1000
 * rounded to f32 */
static double grid(int point, int coord)
{
    if (point < 129)
        return (double)((point * 31 + coord * 17 + point * coord * 7) % 33 - 16) / 8.0;
    return (double)(float)((double)((point * 7919 + coord * 104729 + point * coord * 13) % 4001 - 2000) / 1000.0);
}

/* the lattice of the one-argument cases over [-110, 100], exact in f32: +0, -0, +-2^-30, +-2^-8, 100, then -110 + 13/16 j */
static double lattice(int point, int)
{
    static const double head[] = {0.0, -0.0, 9.313225746154785e-10, -9.313225746154785e-10, 0.00390625, -0.00390625, 100.0};
    constexpr int n_head = (int)(sizeof(head) / sizeof(head[0]));
    return point < n_head ? head[point] : -110.0 + 0.8125 * (double)(point - n_head);
}

template <class T> static void put(FILE *f, const std::vector<T> &v)
{
    if (fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) {
        fprintf(stderr, "short write\n");
        exit(2);
    }
}

template <class T, class F, class H>
static void run_case(FILE *f, const char *name, const double *params, const std::vector<double> &data, double (*point)(int, int))
{
    constexpr int D = F::dim;
    constexpr bool hand = !is_same_type<H, no_hand>::value;
    std::vector<T> bound(data.begin(), data.end()); /* (T)double, exactly data_len elements */
    mm_tparams<T> P;
    for (int i = 0; i < 8; ++i)
        P.p[i] = (T)params[i];
    P.mat = bound.empty() ? nullptr : bound.data();
    std::vector<T> x(N_POINTS * D), va(N_POINTS), vp(N_POINTS), ga(N_POINTS * D), vh(N_POINTS), gh(N_POINTS * D);
    for (int n = 0; n < N_POINTS; ++n) {
        for (int i = 0; i < D; ++i)
            x[n * D + i] = (T)point(n, i);
        va[n] = mm_ad_logp_grad<T, F>(P, &x[n * D], &ga[n * D]);
        vp[n] = F::template logp<T>(P, &x[n * D]);
        if constexpr (hand)
            vh[n] = H::logp_grad(P, &x[n * D], &gh[n * D]);
    }
    printf("%s %s %d %d %ld %d\n", name, sizeof(T) == 4 ? "f32" : "f64", D, N_POINTS, ftell(f), hand ? 1 : 0);
    put(f, x);
    put(f, va);
    put(f, vp);
    put(f, ga);
    if (hand) {
        put(f, vh);
        put(f, gh);
    }
}

template <template <class> class F, template <class> class H>
static void both(FILE *f, const char *name, const double *params, const std::vector<double> &data, double (*point)(int, int))
{
    run_case<float, F<float>, H<float>>(f, name, params, data, point);
    run_case<double, F<double>, H<double>>(f, name, params, data, point);
}

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: %s <out.bin> <data.bin>\n", argv[0]);
        return 2;
    }
    constexpr size_t n_lin = 28, n_logit = 50;
    std::vector<double> all(n_lin + n_logit);
    FILE *d = fopen(argv[2], "rb");
    if (!d || fread(all.data(), sizeof(double), all.size(), d) != all.size()) {
        fprintf(stderr, "%s: expected %zu float64 values\n", argv[2], all.size());
        return 2;
    }
    fclose(d);
    const std::vector<double> lin(all.begin(), all.begin() + n_lin), logit(all.begin() + n_lin, all.end()), nothing;
    FILE *f = fopen(argv[1], "wb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    const double zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const double lin_params[8] = {0.25, 0.25, 0, 0, 0, 0, 0, 0}; /* 1 / sigma^2, 1 / tau^2 (tests/data_common.py) */
    both<linreg3::mmcmc_user_logp, linreg3::mmcmc_user_target>(f, "linreg3", lin_params, lin, grid);
    both<logit9::mmcmc_user_logp, logit9::mmcmc_user_target>(f, "logit9", zero, logit, grid);
    both<softplus::mmcmc_user_logp, none>(f, "softplus", zero, nothing, lattice);
    both<softplus_composed::mmcmc_user_logp, none>(f, "softplus_composed", zero, nothing, lattice);
    both<sigmoid::mmcmc_user_logp, none>(f, "sigmoid", zero, nothing, lattice);
    if (fclose(f) != 0)
        return 2;
    return 0;
}
