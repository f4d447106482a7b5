/* stats_plan.cpp -- the plan of the diagnostics dispatch (csrc/mm_stats_plan.h) walked on the host, the header alone.
 *
 * The grid of tests/cpp/stats_launch_trace.cpp: 6 selectors x f32/f64 x aligned/unaligned sample x with/without wb_part x 27
 * half-chain lengths m on both sides of every threshold x n in {2 m, 2 m + 1} x 11 dimensions x 9 chain counts, the
 * direct-work limit at its default, and the shapes beyond that limit once more with the limit at 0; all of it under four
 * settings of the measurement knobs (main).  For every plan, kChecks
 * checks (each counted whether or not its premise holds):
 *   1-3  every block of the workspace (rows, partial bin totals, their f64 sum) ends inside the size mm_stats_ws_floats gives
 *        for the shape -- which knows no selector, so the buffer an entry point sized fits whichever kernel a racing
 *        mmcmc_stats_set_kernel makes the call run;
 *   4    and so does the total the plan says it uses;
 *   5    the blocks do not overlap;
 *   6    the f64 block starts on an 8-byte boundary;
 *   7    every launch's grid: each dimension in [1, 2^31), y and z at most 65535, at most 1024 threads per block;
 *   8    dynamic LDS at most 160 KB, and beyond 64 KB exactly when the plan says the limit must be raised;
 *   9    the short transform's (r1, dt, wpe) is one of the eight instantiated triples, and its n_pt tiles of dt cover dim;
 *   10   tile1: parts x dim waves are no more than the slabs there are, and the rows are whole groups of parts;
 *   11   a refused call launches nothing and uses no workspace; an accepted one has a first stage and a tail;
 *   12   the status is one of OK / SHAPE / UNSUPPORTED (INVALID_ARG for the zero-sized and mistyped calls added at the end).
 * Prints "plans P", "checks N failed M"; exit status 0 only if M = 0. */
#include "../../mini_mcmc_amd/csrc/mm_stats_plan.h"

#include <cstdio>
#include <initializer_list>

static long g_checks = 0, g_failed = 0;
static const char *g_what = "";
#define CHECK(cond)                                                                                               \
    do {                                                                                                          \
        ++g_checks;                                                                                               \
        if (!(cond) && ++g_failed <= 20)                                                                          \
            std::printf("FAILED %s:%d %s -- %s\n", __FILE__, __LINE__, #cond, g_what);                            \
    } while (0)

static bool grid_ok(const mm_stats_launch &l)
{
    if (l.block == 0) /* no such launch */
        return l.gx == 0;
    return l.gx >= 1 && l.gx < (1u << 31) && l.gy >= 1 && l.gy <= 65535 && l.gz >= 1 && l.gz <= 65535 && l.block <= 1024;
}

static bool triple_ok(const mm_stats_plan &p)
{
    static const int t[8][3] = {{8, 1, 3}, {8, 2, 3}, {8, 3, 3}, {8, 4, 2}, {16, 1, 2}, {16, 2, 2}, {16, 3, 2}, {32, 1, 2}};
    for (const auto &e : t)
        if (p.r1 == e[0] && p.dt == e[1] && p.wpe == e[2])
            return true;
    return false;
}

static mm_stats_knobs g_knobs;

static void check_plan(int sel, int dtype, bool aligned, bool wb, size_t C, size_t n, size_t D, uint64_t limit, bool bad_args = false)
{
    static char what[200];
    std::snprintf(what, sizeof what, "sel %d dtype %d aligned %d wb %d C %zu n %zu D %zu limit %llu knobs %d %d", sel, dtype,
                  (int)aligned, (int)wb, C, n, D, (unsigned long long)limit, g_knobs.fft_nwg_percent, g_knobs.waves);
    g_what = what;
    const mm_stats_knobs k = g_knobs;
    const unsigned int n_parts = 16;
    const mm_stats_plan p = mm_stats_make_plan(C, n, D, dtype, sel, n_parts, wb, aligned, k, limit);
    const size_t ws = mm_stats_ws_floats(C, n, D, n_parts, k);
    const bool ok = p.status == MMCMC_OK;
    CHECK(p.len_slabs <= ws);
    CHECK(p.off_bins + p.len_bins <= ws);
    CHECK(p.off_P + p.len_P <= ws);
    CHECK(p.ws_floats <= ws && p.ws_floats >= p.len_slabs + p.len_bins + p.len_P);
    CHECK(p.len_slabs <= (p.len_bins ? p.off_bins : ws) && p.off_bins + p.len_bins <= (p.len_P ? p.off_P : ws));
    CHECK(p.off_P % 2 == 0 && (p.len_P != 0) == (ok && p.finish_kind == MM_STATS_FINISH_LONG));
    CHECK(grid_ok(p.pre) && grid_ok(p.first) && grid_ok(p.tail) && grid_ok(p.sum) && grid_ok(p.finish));
    CHECK(p.first.lds <= 160 * 1024 && p.finish.lds <= 64 * 1024 && p.raise_lds == (p.first.lds > 64 * 1024) && p.pre.lds == 0 &&
          p.tail.lds == 0 && p.sum.lds == 0);
    CHECK(!(ok && p.path == MM_STATS_FFT) || (triple_ok(p) && (size_t)p.arg * p.dt >= D && p.first.gx % p.arg == 0));
    CHECK(!(ok && p.path == MM_STATS_TILE1) || ((size_t)p.arg * D <= stats_n_slabs(C, k) && p.arg >= 1 && p.rows % p.arg == 0 &&
                                                 n / 2 <= 512));
    if (ok)
        CHECK(p.first.block != 0 && p.tail.block != 0 && p.rows >= 1 && p.row_len >= 1 && p.nb_red >= 1 &&
              p.writes_total == (p.finish_kind != MM_STATS_FINISH_NONE) && (p.finish.block != 0) == p.writes_total &&
              (p.sum.block != 0) == (p.finish_kind == MM_STATS_FINISH_LONG));
    else
        CHECK(p.pre.block == 0 && p.first.block == 0 && p.tail.block == 0 && p.sum.block == 0 && p.finish.block == 0 &&
              p.ws_floats == 0 && !p.writes_total);
    CHECK(bad_args ? p.status == MMCMC_ERR_INVALID_ARG
                   : p.status == MMCMC_OK || p.status == MMCMC_ERR_SHAPE || p.status == MMCMC_ERR_UNSUPPORTED);
}

int main()
{
    constexpr int kChecks = 12;
    static const size_t kM[] = {1,    2,    3,    50,   100,  101,  180,  256,   257,   400,   512,    513,   800,  1024,
                                1025, 1500, 2048, 2049, 2500, 3072, 3073, 8000,  16384, 16385, 65000,  131072, 131073};
    static const size_t kD[] = {1, 3, 4, 5, 12, 13, 16, 17, 33, 4097, 65537};
    static const size_t kC[] = {1, 2, 3, 9, 1000, 2048, 2049, 65536, (size_t)1 << 26};
    const uint64_t kLimit = 1ull << 46;
    long plans = 0, beyond = 0;
    /* the measurement knobs: not set; no workgroups asked for (one is launched) and 7 waves; 2.5 x the workgroups and more
     * waves than any chain count but the largest has half-chains; half the workgroups and 4096 waves without the paths' caps */
    for (const mm_stats_knobs &knobs : {mm_stats_knobs{}, mm_stats_knobs{0, 7}, mm_stats_knobs{250, 200000}, mm_stats_knobs{50, 4096}}) {
    g_knobs = knobs;
    for (int sel = MMCMC_STATS_KERNEL_AUTO; sel <= MMCMC_STATS_KERNEL_DIRECT; ++sel)
        for (int dtype : {MMCMC_F32, MMCMC_F64})
            for (bool aligned : {true, false})
                for (bool wb : {true, false})
                    for (size_t m : kM)
                        for (size_t n : {2 * m, 2 * m + 1})
                            for (size_t D : kD)
                                for (size_t C : kC) {
                                    check_plan(sel, dtype, aligned, wb, C, n, D, kLimit);
                                    ++plans;
                                    /* refused for the work alone: the same shape with the limit lifted has a plan to check */
                                    if (mm_stats_make_plan(C, n, D, dtype, sel, 16, wb, aligned, g_knobs, kLimit).status ==
                                        MMCMC_ERR_UNSUPPORTED) {
                                        check_plan(sel, dtype, aligned, wb, C, n, D, 0);
                                        ++plans, ++beyond;
                                    }
                                }
    }
    for (int sel = MMCMC_STATS_KERNEL_AUTO; sel <= MMCMC_STATS_KERNEL_DIRECT; ++sel) {
        check_plan(sel, MMCMC_F32, true, true, 0, 400, 3, kLimit, true);
        check_plan(sel, MMCMC_F32, true, true, 9, 400, 0, kLimit, true);
        check_plan(sel, 7, true, true, 9, 400, 3, kLimit, true);
        plans += 3;
    }
    std::printf("plans %ld beyond_limit %ld\n", plans, beyond);
    std::printf("checks %ld failed %ld\n", g_checks, g_failed);
    return g_failed == 0 && g_checks == plans * kChecks ? 0 : 1;
}
