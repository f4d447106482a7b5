// Exercises the HMC field setters and run_scheduled of include/mmcmc.hpp.  Built and run by tests/test_hmc_fields.py;
// needs a GPU to go past the constructor, and checks the loud failure (MMCMC_ERR_NO_DEVICE) when there is none.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mmcmc.hpp"

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
        HMC<float> a(RosenbrockND(3), init, n, 0.02f, 10);
        REQUIRE(expect_gpu);
        HMC<float> b(RosenbrockND(3), init, n, 0.02f, 10);
        a.set_seed(5);
        b.set_seed(5);
        // transition k uses (eps[k], L[k]); the first 4 are discarded
        const std::vector<double> eps = {0.01, 0.02, 0.02, 0.005, 0.03, 0.011, 0.011, 0.011, 0.017, 0.02};
        const std::vector<int32_t> nl = {3, 10, 10, 0, 7, 12, 12, 1, 10, 4};
        auto s = a.run_scheduled(eps, nl, 6);
        REQUIRE(s.size() == n * 6 * 3);
        REQUIRE(a.step_size() == (double)0.02f && a.n_leapfrog() == 10);
        std::vector<float> loop;
        for (size_t k = 0; k < eps.size(); ++k) {
            b.set_step_size(eps[k]).set_n_leapfrog(nl[k]);
            b.step();
            if (k >= 4) {
                auto p = b.positions();
                loop.insert(loop.end(), p.begin(), p.end());
            }
        }
        for (size_t c = 0; c < n; ++c)
            for (size_t r = 0; r < 6; ++r)
                for (size_t i = 0; i < 3; ++i)
                    REQUIRE(s[(c * 6 + r) * 3 + i] == loop[(r * n + c) * 3 + i]);
        REQUIRE(a.positions() == b.positions());
        // positions: set and read back
        auto x1 = init_with_seed<float>(n, 3, 9);
        a.set_positions(x1);
        REQUIRE(a.positions() == x1);
        bool threw = false;
        try {
            a.set_step_size(-1.0);
        } catch (const Error &e) {
            threw = e.status == MMCMC_ERR_INVALID_ARG;
        }
        REQUIRE(threw);
        std::printf("hmc fields ok (gpu)\n");
        return 0;
    } catch (const Error &e) {
        if (!expect_gpu && e.status == MMCMC_ERR_NO_DEVICE) {
            std::printf("hmc fields ok (no gpu: %s)\n", e.what());
            return 0;
        }
        std::printf("unexpected error: %s\n", e.what());
        return 2;
    }
}
