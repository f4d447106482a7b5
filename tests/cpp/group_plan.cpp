/* group_plan.cpp -- the host rules of a device group (csrc/mm_group_plan.h) walked exhaustively on the host.
 *
 *  (a) the partition, for every n_devices in 1..64 and n_chains in n_devices..n_devices + 130: the shards are contiguous,
 *      cover [0, n_chains), differ in size by at most one with the larger ones first, and cmax is the largest; 1000 chains
 *      on three devices are 334 + 333 + 333 (tests/test_device_group.py);
 *  (b) the exchange status over all eight combinations of (device listed twice, library accepts shared devices, collectives
 *      found) against the four documented values, and the -2 of a failed communicator initialisation;
 *  (c) both break rules for every (n_advanced, N) with N <= 8 and a status that is OK or an error: never broken on OK;
 *      blocking: broken exactly when some but not all shards advanced; asynchronous: exactly when one was enqueued.
 * Prints the number of cases walked; exit status 0 only if every check held. */
#include "../../mini_mcmc_amd/csrc/mm_group_plan.h"

#include <cstdio>
#include <initializer_list>

static long g_failed = 0;
#define CHECK(cond, ...)                                                                                          \
    do {                                                                                                          \
        if (!(cond)) {                                                                                            \
            if (++g_failed <= 20) {                                                                               \
                std::printf("FAILED %s:%d %s -- ", __FILE__, __LINE__, #cond);                                    \
                std::printf(__VA_ARGS__);                                                                         \
                std::printf("\n");                                                                                \
            }                                                                                                     \
        }                                                                                                         \
    } while (0)

static long partitions()
{
    long n = 0;
    for (size_t N = 1; N <= 64; ++N)
        for (size_t C = N; C <= N + 130; ++C, ++n) {
            size_t next = 0, largest = 0, prev = 0;
            for (size_t i = 0; i < N; ++i) {
                const mm_group_slice s = mm_group_partition(C, N, i);
                CHECK(s.first == next, "C %zu N %zu shard %zu starts at %zu, not %zu", C, N, i, s.first, next);
                CHECK(s.n >= 1, "C %zu N %zu shard %zu is empty", C, N, i);
                CHECK(i == 0 || s.n <= prev, "C %zu N %zu shard %zu is larger than the one before", C, N, i);
                next = s.first + s.n;
                largest = s.n > largest ? s.n : largest;
                prev = s.n;
            }
            CHECK(next == C, "C %zu N %zu covers %zu chains", C, N, next);
            CHECK(largest - prev <= 1, "C %zu N %zu sizes %zu .. %zu", C, N, prev, largest); /* prev: the last = the smallest */
            CHECK(mm_group_cmax(C, N) == largest, "C %zu N %zu cmax %zu, largest %zu", C, N, mm_group_cmax(C, N), largest);
        }
    const size_t want[3][2] = {{0, 334}, {334, 333}, {667, 333}};
    for (size_t i = 0; i < 3; ++i) {
        const mm_group_slice s = mm_group_partition(1000, 3, i);
        CHECK(s.first == want[i][0] && s.n == want[i][1], "1000 / 3 shard %zu: [%zu, +%zu)", i, s.first, s.n);
    }
    CHECK(mm_group_cmax(1000, 3) == 334, "1000 / 3");
    return n;
}

static long duplicates()
{
    long n = 0;
    /* every list of up to four devices out of {0, 1, 2}, against a count of each ordinal */
    for (int len = 1; len <= 4; ++len) {
        int total = 1;
        for (int k = 0; k < len; ++k)
            total *= 3;
        for (int code = 0; code < total; ++code, ++n) {
            int dev[4], seen[3] = {0, 0, 0}, c = code;
            bool dup = false;
            for (int k = 0; k < len; ++k, c /= 3) {
                dev[k] = c % 3;
                dup = dup || seen[dev[k]]++ > 0;
            }
            CHECK(mm_group_has_duplicate(dev, len) == dup, "len %d code %d", len, code);
        }
    }
    return n;
}

static long exchanges()
{
    long n = 0;
    /* by bits = dup | share << 1 | ok << 2.  1: the collectives, found and allowed on these devices; 0: a device twice and no
     * library that takes that (also when none was found at all: a library that is not there does not take it either);
     * -1: distinct devices, no library */
    static const int table[8] = {-1, 0, -1, 0, 1, 0, 1, 1};
    for (int bits = 0; bits < 8; ++bits, ++n) {
        const bool dup = bits & 1, share = bits & 2, ok = bits & 4;
        const mm_group_exchange_plan p = mm_group_exchange(dup, share, ok);
        const int want = table[bits];
        CHECK(p.status == want, "dup %d share %d ok %d: status %d, not %d", dup, share, ok, p.status, want);
        CHECK(p.use_rccl == (p.status == 1), "dup %d share %d ok %d: use_rccl %d with status %d", dup, share, ok, p.use_rccl, p.status);
    }
    /* the documented values, case by case */
    CHECK(mm_group_exchange(false, false, true).status == 1, "distinct devices, RCCL");
    CHECK(mm_group_exchange(true, false, true).status == 0, "a device twice under RCCL: the host by design");
    CHECK(mm_group_exchange(true, true, true).status == 1, "a device twice under a library that takes it");
    CHECK(mm_group_exchange(false, false, false).status == -1, "no library: the host as a fallback");
    const mm_group_exchange_plan f = mm_group_exchange_init_failed();
    CHECK(f.status == -2 && !f.use_rccl, "ncclCommInitAll failed");
    return n;
}

static long breaks()
{
    long n = 0;
    for (size_t N = 1; N <= 8; ++N)
        for (size_t adv = 0; adv <= N; ++adv)
            for (int status : {MMCMC_OK, MMCMC_ERR_NO_DEVICE, 2 /* a HIP error passed through */}) {
                ++n;
                const bool failed = status != MMCMC_OK;
                CHECK(mm_group_breaks_blocking(adv, N, status) == (failed && adv > 0 && adv < N), "blocking: %zu of %zu, status %d", adv, N, status);
                CHECK(mm_group_breaks_async(adv, status) == (failed && adv > 0), "async: %zu of %zu, status %d", adv, N, status);
            }
    return n;
}

int main()
{
    const long p = partitions(), d = duplicates(), e = exchanges(), b = breaks();
    std::printf("partitions %ld device lists %ld exchanges %ld break cases %ld failed %ld\n", p, d, e, b, g_failed);
    return g_failed ? 1 : 0;
}
