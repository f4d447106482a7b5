// Exercises the chain-state setters and stream positions of include/mmcmc.hpp (checkpoint and resume).  Built and run by
// tests/test_resume.py; needs a GPU to go past the first constructor, and checks the loud failure (MMCMC_ERR_NO_DEVICE)
// when there is none.  With a GPU: a handle given another's positions, fields and stream position continues exactly as
// that one does.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mmcmc.hpp"

// every member of the facade's class templates compiles, used here or not
template class mmcmc::MetropolisHastings<float>;
template class mmcmc::HMC<double>;
template class mmcmc::HMCGroup<float>;
template class mmcmc::NUTS<double>;
template class mmcmc::NUTSGroup<float>;

#define REQUIRE(c)                                                                                                 \
    do {                                                                                                           \
        if (!(c)) {                                                                                                \
            std::printf("FAILED: %s (line %d)\n", #c, __LINE__);                                                   \
            return 1;                                                                                              \
        }                                                                                                          \
    } while (0)

int main(int argc, char **argv)
{
    using namespace mmcmc;
    const bool expect_gpu = argc > 1 && std::atoi(argv[1]) != 0;
    const size_t n = 256;
    auto init = init_with_seed<float>(n, 3, 42);
    try {
        MetropolisHastings<float> a(RosenbrockND(3), IsotropicGaussian(0.5), init, n);
        REQUIRE(expect_gpu);
        MetropolisHastings<float> b(RosenbrockND(3), IsotropicGaussian(1.5), init_with_seed<float>(n, 3, 7), n);
        a.seed(5).set_proposal_std(0.25);
        b.seed(9);
        a.run(10, 5);
        const StreamPosition p = a.stream_position();
        REQUIRE(p.seed == 5 && p.chain_offset == 0 && p.iteration == 15);
        const auto x = a.positions();
        auto sa = a.run(20, 3);
        b.seed(p.seed).set_iteration(p.iteration).set_proposal_std(a.proposal_std()).set_positions(x);
        auto sb = b.run(20, 3);
        REQUIRE(sa == sb && a.positions() == b.positions());
        REQUIRE(b.stream_position().iteration == 38);

        // NUTS in f64: positions and adaptation records round-trip exactly; the continuation is the same
        std::vector<double> init64(init.begin(), init.end());
        NUTS64 c(RosenbrockND(3), init64, n, 0.8), d(RosenbrockND(3), init_with_seed<double>(n, 3, 3), n, 0.8);
        c.set_seed(11);
        c.run(5, 20);
        const StreamPosition q = c.stream_position();
        const auto ad = c.adapt_state();
        const auto xc = c.positions();
        auto sc = c.run(10, 40);
        d.set_seed(q.seed).set_iteration(q.iteration).set_positions(xc).set_adapt_state(ad);
        REQUIRE(d.adapt_state() == ad);
        auto sd = d.run(10, 40);
        REQUIRE(sc == sd && c.adapt_state() == d.adapt_state());
        bool threw = false;
        try {
            a.set_proposal_std(0.0);
        } catch (const Error &e) {
            threw = e.status == MMCMC_ERR_INVALID_ARG;
        }
        REQUIRE(threw && a.proposal_std() == 0.25);
        std::printf("resume ok (gpu)\n");
        return 0;
    } catch (const Error &e) {
        if (!expect_gpu && e.status == MMCMC_ERR_NO_DEVICE) {
            std::printf("resume ok (no gpu: %s)\n", e.what());
            return 0;
        }
        std::printf("unexpected error: %s\n", e.what());
        return 2;
    }
}
