/* path_rule.cpp -- the kernel-path rule of an MH / HMC handle (csrc/mm_path.h) walked exhaustively on the host.
 *
 * Every combination of the mm_path_caps fields (both samplers, both dtypes, dim in {1, 8, 9, 16, 17, 32, 33, 128}, every
 * boolean, every unit state) that sampler_create can produce (mm_path_caps_consistent: the others describe no handle, e.g.
 * the launchers of a table entry that does not exist, or no kernel at all), every variant from -1 to 9:
 *  (a) the default variant has status OK;
 *  (b) for every variant with status OK, n_leapfrog in {0, 9, 10} and scheduled in {false, true}: the launcher named by
 *      mm_launch_path exists on the handle -- no path reaches a null function pointer;
 *  (c) every other variant yields exactly INVALID_ARG or UNSUPPORTED;
 *  (d) the quirks the public API has always had, each as an explicit case.
 * Prints the number of handles and (handle, variant, L, scheduled) tuples walked; exit status 0 only if every check held. */
#include "../../mini_mcmc_amd/csrc/mm_path.h"

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

/* does the handle have the launcher? (what launch_range dereferences or calls for each enumerator) */
static bool launcher_exists(const mm_path_caps &c, mm_launch p)
{
    switch (p) {
    case MM_LAUNCH_PLAIN:
    case MM_LAUNCH_PP:
    case MM_LAUNCH_PP10:
        return c.fixed;
    case MM_LAUNCH_SPLIT:
    case MM_LAUNCH_SPLIT10:
        return c.fixed && c.split;
    case MM_LAUNCH_PP_SCHED:
        return c.fixed && c.pp_sched && c.sampler == MM_SAMPLER_HMC;
    case MM_LAUNCH_SPLIT_SCHED:
        return c.fixed && c.split_sched && c.sampler == MM_SAMPLER_HMC;
    case MM_LAUNCH_UNIT:
        return c.unit != MM_UNIT_NONE;
    case MM_LAUNCH_GENERIC: /* next to a fixed kernel there is no HBM store: the chain vectors must fit LDS */
        return c.generic_ok && (c.generic_lds || !c.fixed);
    case MM_LAUNCH_WIDE:
        return c.wide_ok;
    case MM_LAUNCH_LG:
        return c.lg_ok;
    case MM_LAUNCH_SEGMENTED: /* no launcher of its own: sampler_run splits the run into unscheduled launches */
        return true;
    }
    return false;
}

static void describe(const mm_path_caps &c, char *buf, size_t n)
{
    std::snprintf(buf, n, "sampler %d dtype %d dim %d fixed %d split %d pp_sched %d split_sched %d unit %d generic_ok %d generic_lds %d wide %d lg %d few %d",
                  c.sampler, c.dtype, c.dim, c.fixed, c.split, c.pp_sched, c.split_sched, (int)c.unit, c.generic_ok, c.generic_lds,
                  c.wide_ok, c.lg_ok, c.few_chains);
}

static mm_path_caps handle(int sampler, int dtype, int dim)
{
    mm_path_caps c;
    c.sampler = sampler;
    c.dtype = dtype;
    c.dim = dim;
    return c;
}

/* (d): the quirks, on the caps of the handles that show them */
static void quirks()
{
    /* RosenbrockND(3) f32: a fixed entry with every launcher */
    mm_path_caps f = handle(MM_SAMPLER_HMC, MMCMC_F32, 3);
    f.fixed = f.split = f.pp_sched = f.split_sched = f.generic_ok = f.generic_lds = true;
    for (int sampler : {MM_SAMPLER_MH, MM_SAMPLER_HMC}) {
        f.sampler = sampler;
        /* variant 1 is accepted as itself (the setter stores what it was given) and runs PIPE = 2 */
        CHECK(mm_variant_status(f, 1) == MMCMC_OK, "sampler %d", sampler);
        CHECK(mm_launch_path(f, 1, 9, false) == MM_LAUNCH_PP && mm_launch_path(f, 2, 9, false) == MM_LAUNCH_PP, "sampler %d", sampler);
        /* variant 7 without a unit: OK, runs pp (pp10 at L = 10 under HMC), segmented when scheduled */
        CHECK(mm_variant_status(f, 7) == MMCMC_OK, "sampler %d", sampler);
        CHECK(mm_launch_path(f, 7, 9, false) == MM_LAUNCH_PP, "sampler %d", sampler);
        CHECK(mm_launch_path(f, 7, 10, false) == (sampler == MM_SAMPLER_HMC ? MM_LAUNCH_PP10 : MM_LAUNCH_PP), "sampler %d", sampler);
        CHECK(mm_launch_path(f, 7, 10, true) == MM_LAUNCH_SEGMENTED, "sampler %d", sampler);
        /* the ranges: MH refuses 3, 4 and 8, HMC refuses 4, both anything below 0 or above 8 */
        for (int v = -1; v <= 9; ++v) {
            const bool invalid = v < 0 || v > 8 || v == 4 || (sampler == MM_SAMPLER_MH && (v == 3 || v == 8));
            CHECK((mm_variant_status(f, v) == MMCMC_ERR_INVALID_ARG) == invalid, "sampler %d variant %d", sampler, v);
        }
    }
    f.sampler = MM_SAMPLER_HMC;
    CHECK(mm_default_variant(f) == 5 && mm_launch_path(f, 1, 10, true) == MM_LAUNCH_PP_SCHED && mm_launch_path(f, 5, 10, true) == MM_LAUNCH_SPLIT_SCHED, "scheduled kernels");
    CHECK(mm_launch_path(f, 0, 10, true) == MM_LAUNCH_SEGMENTED && mm_launch_path(f, 6, 10, true) == MM_LAUNCH_SEGMENTED, "no scheduled kernel");
    /* a caller's unit: 7 and nothing else */
    mm_path_caps u = handle(MM_SAMPLER_HMC, MMCMC_F32, 2);
    u.unit = MM_UNIT_CALLER;
    CHECK(mm_default_variant(u) == 7, "caller's unit");
    for (int v = 0; v <= 8; ++v)
        if (v != 4)
            CHECK(mm_variant_status(u, v) == (v == 7 ? MMCMC_OK : MMCMC_ERR_UNSUPPORTED), "caller's unit, variant %d", v);
    CHECK(mm_launch_path(u, 7, 10, false) == MM_LAUNCH_UNIT && mm_launch_path(u, 7, 10, true) == MM_LAUNCH_SEGMENTED, "caller's unit");
    /* a built-in's unit (RosenbrockND(9)): 6 and 7 only */
    mm_path_caps b = handle(MM_SAMPLER_HMC, MMCMC_F64, 9);
    b.unit = MM_UNIT_BUILTIN;
    b.generic_ok = b.generic_lds = true;
    CHECK(mm_default_variant(b) == 7, "built-in's unit");
    for (int v = 0; v <= 8; ++v)
        if (v != 4)
            CHECK(mm_variant_status(b, v) == (v == 6 || v == 7 ? MMCMC_OK : MMCMC_ERR_UNSUPPORTED), "built-in's unit, variant %d", v);
    CHECK(mm_launch_path(b, 6, 3, false) == MM_LAUNCH_GENERIC && mm_launch_path(b, 7, 3, false) == MM_LAUNCH_UNIT, "built-in's unit");
    /* ... and once the unit failed its self-check: the run-time-dimension kernel only */
    b.unit = MM_UNIT_NONE;
    CHECK(mm_default_variant(b) == 6 && mm_variant_status(b, 7) == MMCMC_ERR_UNSUPPORTED && mm_variant_status(b, 6) == MMCMC_OK, "unit refused");
    /* 8 is asked before "no fixed kernel: only 6": RosenbrockND(128) under HMC takes 6 and 8, and defaults to 8 with few chains */
    mm_path_caps w = handle(MM_SAMPLER_HMC, MMCMC_F32, 128);
    w.generic_ok = w.generic_lds = w.wide_ok = true;
    CHECK(mm_variant_status(w, 8) == MMCMC_OK && mm_variant_status(w, 6) == MMCMC_OK && mm_variant_status(w, 2) == MMCMC_ERR_UNSUPPORTED, "wide");
    CHECK(mm_default_variant(w) == 6, "1024 chains or more");
    w.few_chains = true;
    CHECK(mm_default_variant(w) == 8 && mm_launch_path(w, 8, 10, false) == MM_LAUNCH_WIDE, "few chains");
    /* the wide kernel next to a fixed one (RosenbrockND(16)): selectable, never the default */
    mm_path_caps w16 = handle(MM_SAMPLER_HMC, MMCMC_F32, 16);
    w16.fixed = w16.pp_sched = w16.generic_ok = w16.generic_lds = w16.wide_ok = true;
    CHECK(mm_default_variant(w16) == 2 && mm_variant_status(w16, 8) == MMCMC_OK, "wide next to a fixed kernel");
    w16.dim = 32; /* plain above dim 16 */
    w16.pp_sched = false;
    CHECK(mm_default_variant(w16) == 0 && mm_launch_path(w16, 2, 9, true) == MM_LAUNCH_SEGMENTED, "dim 32");
    /* the lane-group kernel: the default of a dense Gaussian at 16 / 32 under HMC, refused elsewhere */
    w16.lg_ok = true;
    CHECK(mm_default_variant(w16) == 3 && mm_launch_path(w16, 3, 9, false) == MM_LAUNCH_LG, "lane groups");
    CHECK(mm_variant_status(f, 3) == MMCMC_ERR_UNSUPPORTED, "lane groups without the kernel");
    /* f64 has the split kernels up to dim 8 but not as its default */
    mm_path_caps d = f;
    d.dtype = MMCMC_F64;
    d.split_sched = false;
    CHECK(mm_default_variant(d) == 2 && mm_variant_status(d, 5) == MMCMC_OK && mm_launch_path(d, 5, 10, false) == MM_LAUNCH_SPLIT10 &&
              mm_launch_path(d, 5, 10, true) == MM_LAUNCH_SEGMENTED, "f64 split");
}

int main()
{
    static const int dims[] = {1, 8, 9, 16, 17, 32, 33, 128};
    long handles = 0, combos = 0, tuples = 0;
    char buf[256];
    for (int sampler : {MM_SAMPLER_MH, MM_SAMPLER_HMC})
        for (int dtype : {MMCMC_F32, MMCMC_F64})
            for (int dim : dims)
                for (int bits = 0; bits < (1 << 9); ++bits)
                    for (int unit = MM_UNIT_NONE; unit <= MM_UNIT_BUILTIN; ++unit) {
                        mm_path_caps c = handle(sampler, dtype, dim);
                        c.fixed = bits & 1;
                        c.split = bits & 2;
                        c.pp_sched = bits & 4;
                        c.split_sched = bits & 8;
                        c.generic_ok = bits & 16;
                        c.generic_lds = bits & 32;
                        c.wide_ok = bits & 64;
                        c.lg_ok = bits & 128;
                        c.few_chains = bits & 256;
                        c.unit = (mm_unit_state)unit;
                        ++combos;
                        if (!mm_path_caps_consistent(c))
                            continue;
                        ++handles;
                        describe(c, buf, sizeof buf);
                        const int def = mm_default_variant(c);
                        CHECK(mm_variant_status(c, def) == MMCMC_OK, "default %d of %s", def, buf); /* (a) */
                        for (int v = -1; v <= 9; ++v) {
                            const int st = mm_variant_status(c, v);
                            if (st != MMCMC_OK) {
                                CHECK(st == MMCMC_ERR_INVALID_ARG || st == MMCMC_ERR_UNSUPPORTED, "status %d of variant %d, %s", st, v, buf); /* (c) */
                                continue;
                            }
                            for (int L : {0, 9, 10})
                                for (int scheduled = 0; scheduled < 2; ++scheduled) {
                                    const mm_launch p = mm_launch_path(c, v, L, scheduled != 0);
                                    ++tuples;
                                    CHECK(launcher_exists(c, p), "variant %d L %d scheduled %d -> launcher %d, %s", v, L, scheduled, (int)p, buf); /* (b) */
                                    /* a scheduled kernel only for a scheduled run, the segmented path only for one without */
                                    CHECK(scheduled == (p == MM_LAUNCH_PP_SCHED || p == MM_LAUNCH_SPLIT_SCHED || p == MM_LAUNCH_SEGMENTED),
                                          "variant %d scheduled %d -> launcher %d, %s", v, scheduled, (int)p, buf);
                                }
                        }
                    }
    quirks();
    std::printf("combinations %ld handles %ld tuples %ld failed %ld\n", combos, handles, tuples, g_failed);
    return g_failed ? 1 : 0;
}
