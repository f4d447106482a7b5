/* Host evaluation of the forward-mode gradients of csrc/mm_autodiff.h (tests/test_autodiff_host.py, tests/test_autodiff_gpu.py).
 *
 * Plain C++ with the flags of the host twin (-ffp-contract=off): the same functor code the device runs, so the file this
 * program writes is what mmcmc_logp_grad_batch must return bit for bit.  The log-densities live in autodiff_cases/ (one
 * file per body, each defining mmcmc_user_logp<T>); the tests register those very files on the device.
 *
 * usage: autodiff_host <out.bin>
 * For every case and element type the program appends to <out.bin>, as raw little-endian arrays of that type,
 *     x[n][dim]  value_ad[n]  value_plain[n]  grad_ad[n][dim]  and, where a hand-written gradient exists,  value_hand[n]  grad_hand[n][dim]
 * and prints one index line:  <case> <f32|f64> <dim> <n> <byte offset> <0|1: hand-written gradient present>
 */
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../mini_mcmc_amd/csrc/mm_autodiff.h"

namespace ros2 {
#define MM_USER_DIM 2
#include "autodiff_cases/rosenbrock.inc"
#undef MM_USER_DIM
} // namespace ros2
namespace ros3 {
#define MM_USER_DIM 3
#include "autodiff_cases/rosenbrock.inc"
#undef MM_USER_DIM
} // namespace ros3
namespace ros8 {
#define MM_USER_DIM 8
#include "autodiff_cases/rosenbrock.inc"
#undef MM_USER_DIM
} // namespace ros8
namespace ros9 {
#define MM_USER_DIM 9
#include "autodiff_cases/rosenbrock.inc"
#undef MM_USER_DIM
} // namespace ros9
namespace ros17 {
#define MM_USER_DIM 17
#include "autodiff_cases/rosenbrock.inc"
#undef MM_USER_DIM
} // namespace ros17
namespace ros32 {
#define MM_USER_DIM 32
#include "autodiff_cases/rosenbrock.inc"
#undef MM_USER_DIM
} // namespace ros32
namespace banana {
#include "autodiff_cases/banana.inc"
}
namespace op_div {
#include "autodiff_cases/div.inc"
}
namespace op_log {
#include "autodiff_cases/log.inc"
}
namespace op_exp {
#include "autodiff_cases/exp.inc"
}
namespace op_sqrt {
#include "autodiff_cases/sqrt.inc"
}
namespace op_abs {
#include "autodiff_cases/abs.inc"
}
namespace op_branch {
#include "autodiff_cases/branch.inc"
}

/* the hand-derived gradient of the banana (tests/test_user_target.py: BANANA), the known-good code its bound is tried on */
template <class T> struct banana_hand {
    static constexpr int dim = 2;
    static T logp_grad(const mm_tparams<T> &P, const T *x, T *g)
    {
        const T r = x[1] - P.p[1] * x[0] * x[0];
        g[0] = -x[0] / (P.p[0] * P.p[0]) + T(2) * P.p[1] * x[0] * r;
        g[1] = -r;
        return T(-0.5) * (x[0] * x[0] / (P.p[0] * P.p[0]) + r * r);
    }
};
struct no_hand {};
template <class A, class B> struct is_same_type { static constexpr bool value = false; };
template <class A> struct is_same_type<A, A> { static constexpr bool value = true; };

constexpr int N_POINTS = 257;

/* the fixed grid, |x| <= 2, every coordinate exactly representable in f32: the first 129 points are multiples of 1/8 (every
 * operation of the polynomial densities is then exact in f64), the others multiples of 1/1000 rounded to f32 */
static double grid(int point, int coord)
{
    if (point < 129)
        return (double)((point * 31 + coord * 17 + point * coord * 7) % 33 - 16) / 8.0;
    return (double)(float)((double)((point * 7919 + coord * 104729 + point * coord * 13) % 4001 - 2000) / 1000.0);
}

template <class T> static void put(FILE *f, const std::vector<T> &v)
{
    if (fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) {
        fprintf(stderr, "short write\n");
        exit(2);
    }
}

template <class T, class F, class H> static void run_case(FILE *f, const char *name, const double *params)
{
    constexpr int D = F::dim;
    constexpr bool hand = !is_same_type<H, no_hand>::value;
    mm_tparams<T> P;
    for (int i = 0; i < 8; ++i)
        P.p[i] = (T)params[i];
    P.mat = nullptr;
    std::vector<T> x(N_POINTS * D), va(N_POINTS), vp(N_POINTS), ga(N_POINTS * D), vh(N_POINTS), gh(N_POINTS * D);
    for (int n = 0; n < N_POINTS; ++n) {
        for (int i = 0; i < D; ++i)
            x[n * D + i] = (T)grid(n, i);
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

template <template <class> class F, template <class> class H> static void both(FILE *f, const char *name, const double *params)
{
    run_case<float, F<float>, H<float>>(f, name, params);
    run_case<double, F<double>, H<double>>(f, name, params);
}
template <class T> using none = no_hand;
template <int D> struct ros_hand {
    template <class T> using type = mm_target<T, MM_ROSENBROCK_ND, D>;
};

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: %s <out.bin>\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "wb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    const double zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const double sb[8] = {1.5, 0.5, 0, 0, 0, 0, 0, 0}; /* s, b of test_new_density_samples_what_it_describes */
    both<ros2::mmcmc_user_logp, ros_hand<2>::type>(f, "rosenbrock2", zero);
    both<ros3::mmcmc_user_logp, ros_hand<3>::type>(f, "rosenbrock3", zero);
    both<ros8::mmcmc_user_logp, ros_hand<8>::type>(f, "rosenbrock8", zero);
    both<ros9::mmcmc_user_logp, ros_hand<9>::type>(f, "rosenbrock9", zero);
    both<ros17::mmcmc_user_logp, ros_hand<17>::type>(f, "rosenbrock17", zero);
    both<ros32::mmcmc_user_logp, ros_hand<32>::type>(f, "rosenbrock32", zero);
    both<banana::mmcmc_user_logp, banana_hand>(f, "banana", sb);
    both<op_div::mmcmc_user_logp, none>(f, "div", zero);
    both<op_log::mmcmc_user_logp, none>(f, "log", zero);
    both<op_exp::mmcmc_user_logp, none>(f, "exp", zero);
    both<op_sqrt::mmcmc_user_logp, none>(f, "sqrt", zero);
    both<op_abs::mmcmc_user_logp, none>(f, "abs", zero);
    both<op_branch::mmcmc_user_logp, none>(f, "branch", zero);
    if (fclose(f) != 0)
        return 2;
    return 0;
}
