/* nuts_plan.cpp -- the host rules of a NUTS handle (csrc/mm_nuts_plan.h) walked exhaustively on the host.
 *
 *  (a) the step plan for every (n_collect, n_discard) in 0..6 x 0..6 and progress in -1..3: rows written, transitions taken,
 *      the progress range, and both shape limits at their exact edges;
 *  (b) the path rule over every consistent caps combination x metric kind x recording x variant -1..9: the default is accepted,
 *      an accepted variant never names a launcher the handle lacks, a metric or recording leaves variant 7 and the matching
 *      unit alone, everything else is INVALID_ARG outside 0..7 and UNSUPPORTED inside;
 *  (c) the lane-group mode at its thresholds, the scheduler's grid over groups16 1..4200 x resident waves x occupancy x knobs,
 *      the level rule at the histogram threshold and both clamps;
 *  (d) the pilot split over n_pre 0..40 x n_rec 0..80 x write_initial x out_t0: the two launches take the same transitions
 *      and write the same rows as the one;
 *  (e) the chain groups of variant 2 over n_chains 1..700 and three large counts x requested groups 0..16: the waves are tiled
 *      exactly once, and every transition writes the row the one-launch kernel would.
 * Prints the number of cases walked; exit status 0 only if every check held. */
#include "../../mini_mcmc_amd/csrc/mm_nuts_plan.h"

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

static long steps()
{
    long n = 0;
    for (size_t nc = 0; nc <= 6; ++nc)
        for (size_t nd = 0; nd <= 6; ++nd)
            for (int progress = -1; progress <= 3; ++progress, ++n) {
                const mm_nuts_steps s = mm_nuts_step_plan(nc, nd, progress, 3, 0);
                if (progress < 0 || progress > 2) {
                    CHECK(s.status == MMCMC_ERR_INVALID_ARG, "nc %zu nd %zu progress %d: status %d", nc, nd, progress, s.status);
                    continue;
                }
                CHECK(s.status == MMCMC_OK, "nc %zu nd %zu progress %d: status %d", nc, nd, progress, s.status);
                const size_t total = nc + nd;
                CHECK(s.n_rows == (progress == 2 ? total : nc), "nc %zu nd %zu progress %d: %zu rows", nc, nd, progress, s.n_rows);
                CHECK(s.n_rows == 0 || s.write_initial + s.n_rec == s.n_rows, "nc %zu nd %zu progress %d: %u + %u rows written, not %zu", nc,
                      nd, progress, s.write_initial, s.n_rec, s.n_rows);
                CHECK(s.write_initial <= 1u, "nc %zu nd %zu progress %d", nc, nd, progress);
                const size_t want = progress ? total : (total ? total - 1 : 0);
                CHECK((size_t)s.n_pre + s.n_rec == want, "nc %zu nd %zu progress %d: %u + %u transitions, not %zu", nc, nd, progress, s.n_pre,
                      s.n_rec, want);
                CHECK(progress != 1 || (s.n_pre == nd && s.n_rec == nc), "nc %zu nd %zu: run_progress discards %u, records %u", nc, nd, s.n_pre, s.n_rec);
                CHECK(progress == 0 || s.write_initial == 0u, "nc %zu nd %zu progress %d writes the initial row", nc, nd, progress);
            }
    /* n_rows * dim < 2^30, with and without the burn-in rows */
    const size_t edge = ((size_t)1 << 30) / 4; /* dim 4 */
    for (int progress = 0; progress <= 2; ++progress, ++n) {
        CHECK(mm_nuts_step_plan(edge - 1, 0, progress, 4, 0).status == MMCMC_OK, "progress %d: 2^30 - 4 elements per chain", progress);
        CHECK(mm_nuts_step_plan(edge, 0, progress, 4, 0).status == MMCMC_ERR_SHAPE, "progress %d: 2^30 elements per chain", progress);
    }
    CHECK(mm_nuts_step_plan(edge - 2, 1, 2, 4, 0).status == MMCMC_OK, "burn-in rows counted");
    CHECK(mm_nuts_step_plan(edge - 1, 1, 2, 4, 0).status == MMCMC_ERR_SHAPE, "burn-in rows counted");
    CHECK(mm_nuts_step_plan(edge - 1, 1, 1, 4, 0).status == MMCMC_OK, "burn-in rows are not written under progress 1");
    /* m + n_collect + n_discard < 2^32 */
    const uint32_t m = 0xfffffff0u;
    CHECK(mm_nuts_step_plan(10, 5, 0, 1, m).status == MMCMC_OK, "2^32 - 1 steps");
    CHECK(mm_nuts_step_plan(10, 6, 0, 1, m).status == MMCMC_ERR_SHAPE, "2^32 steps");
    CHECK(mm_nuts_step_plan(11, 5, 1, 1, m).status == MMCMC_ERR_SHAPE, "2^32 steps");
    CHECK(mm_nuts_step_plan(0, 0, 0, 1, 0xffffffffu).status == MMCMC_OK, "an empty run at the last step");
    CHECK(mm_nuts_step_plan(1, 0, 0, 1, 0xffffffffu).status == MMCMC_ERR_SHAPE, "one more row at the last step");
    /* the range of progress comes before the shape */
    CHECK(mm_nuts_step_plan(edge, 0, 3, 4, 0).status == MMCMC_ERR_INVALID_ARG, "progress 3 on a shape that is too large");
    return n + 10;
}

static bool has(const mm_nuts_caps &c, mm_nuts_launch l, int metric, bool recording)
{
    switch (l) {
    case MM_NLAUNCH_INST_STEP: return c.inst;
    case MM_NLAUNCH_INST_ASYNC: return c.inst && c.inst_async;
    case MM_NLAUNCH_INST_PAIR: return c.inst && c.inst_pair;
    case MM_NLAUNCH_LG: return c.lg;
    case MM_NLAUNCH_GENERIC: return c.generic_ok;
    case MM_NLAUNCH_TARGET_UNIT: return c.unit;
    case MM_NLAUNCH_METRIC_UNIT: return !recording && metric == MM_NMETRIC_DIAG;
    case MM_NLAUNCH_DENSE_UNIT: return !recording && metric == MM_NMETRIC_DENSE;
    case MM_NLAUNCH_STATS_UNIT: return recording && metric == MM_NMETRIC_NONE;
    case MM_NLAUNCH_STATS_UNIT_DIAG: return recording && metric == MM_NMETRIC_DIAG;
    case MM_NLAUNCH_STATS_UNIT_DENSE: return recording && metric == MM_NMETRIC_DENSE;
    default: return false;
    }
}

static long g_handles = 0, g_accepted = 0;
static long paths()
{
    long n = 0;
    for (int bits = 0; bits < 64; ++bits, ++n) {
        mm_nuts_caps c;
        c.inst = bits & 1, c.inst_async = bits & 2, c.inst_pair = bits & 4, c.lg = bits & 8, c.generic_ok = bits & 16, c.unit = bits & 32;
        if (!mm_nuts_caps_consistent(c))
            continue;
        ++g_handles;
        const int d = mm_nuts_default_variant(c);
        /* today's order: 3, 5, 4, 0, 7, 6 */
        const int want_d = c.lg ? 3 : (c.inst && c.inst_pair) ? 5 : (c.inst && c.inst_async) ? 4 : c.inst ? 0 : c.unit ? 7 : 6;
        CHECK(d == want_d, "caps %d: default %d, not %d", bits, d, want_d);
        CHECK(mm_nuts_variant_status(c, MM_NMETRIC_NONE, false, d) == MMCMC_OK, "caps %d: the default %d is refused", bits, d);
        for (int metric = MM_NMETRIC_NONE; metric <= MM_NMETRIC_DENSE; ++metric)
            for (int rec = 0; rec < 2; ++rec)
                for (int v = -1; v <= 9; ++v) {
                    const int st = mm_nuts_variant_status(c, metric, rec != 0, v);
                    const mm_nuts_launch l = mm_nuts_launch_path(c, metric, rec != 0, v);
                    if (st != MMCMC_OK) {
                        CHECK(st == (v >= 0 && v <= 7 ? MMCMC_ERR_UNSUPPORTED : MMCMC_ERR_INVALID_ARG), "caps %d metric %d rec %d v %d: status %d",
                              bits, metric, rec, v, st);
                        CHECK(l == MM_NLAUNCH_NONE, "caps %d metric %d rec %d v %d: refused, yet launcher %d", bits, metric, rec, v, (int)l);
                        continue;
                    }
                    ++g_accepted;
                    CHECK(v >= 0 && v <= 7, "caps %d: variant %d accepted", bits, v);
                    CHECK(has(c, l, metric, rec != 0), "caps %d metric %d rec %d v %d: launcher %d, which the handle lacks", bits, metric, rec, v,
                          (int)l);
                    if (metric != MM_NMETRIC_NONE || rec) {
                        CHECK(v == 7, "caps %d metric %d rec %d: variant %d accepted", bits, metric, rec, v);
                        const mm_nuts_launch want = rec ? (mm_nuts_launch)(MM_NLAUNCH_STATS_UNIT + metric)
                                                        : metric == MM_NMETRIC_DENSE ? MM_NLAUNCH_DENSE_UNIT : MM_NLAUNCH_METRIC_UNIT;
                        CHECK(l == want, "caps %d metric %d rec %d: launcher %d, not %d", bits, metric, rec, (int)l, (int)want);
                    } else {
                        /* the variant numbers, one by one */
                        const mm_nuts_launch want = v == 0 ? MM_NLAUNCH_INST_STEP : v <= 3 ? MM_NLAUNCH_LG : v == 4 ? MM_NLAUNCH_INST_ASYNC
                                                    : v == 5 ? MM_NLAUNCH_INST_PAIR : v == 6 ? MM_NLAUNCH_GENERIC : MM_NLAUNCH_TARGET_UNIT;
                        CHECK(l == want, "caps %d v %d: launcher %d, not %d", bits, v, (int)l, (int)want);
                    }
                }
        /* with a metric or while recording 7 is always accepted, whether or not the target has a unit of its own */
        for (int metric = MM_NMETRIC_NONE; metric <= MM_NMETRIC_DENSE; ++metric)
            for (int rec = 0; rec < 2; ++rec)
                if (metric != MM_NMETRIC_NONE || rec)
                    CHECK(mm_nuts_variant_status(c, metric, rec != 0, 7) == MMCMC_OK, "caps %d metric %d rec %d refuses 7", bits, metric, rec);
    }
    return n;
}

static long schedules()
{
    long n = 0;
    const size_t id_cap = (size_t)1 << MM_LGQ_ID_BITS;
    /* the mode at its thresholds */
    for (int v = 1; v <= 3; ++v)
        for (unsigned int total : {0u, 1u, 64u})
            for (size_t chains : {(size_t)1, (size_t)2047, (size_t)2048, id_cap - 16, id_cap - 15, id_cap}) {
                ++n;
                const size_t c_pad = (chains + 15) / 16 * 16;
                const mm_nuts_lg_sched s = mm_nuts_lg_mode(v, total, chains, c_pad);
                const mm_nuts_lg_sched want = (v == 1 || total == 0) ? MM_NLG_SINGLE
                                              : v == 2               ? MM_NLG_PER_LEVEL
                                              : chains < 2048        ? MM_NLG_SINGLE
                                              : c_pad < id_cap       ? MM_NLG_QUEUE
                                                                     : MM_NLG_PER_LEVEL;
                CHECK(s == want, "variant %d total %u chains %zu: mode %d, not %d", v, total, chains, (int)s, (int)want);
            }
    /* the scheduler's grid */
    for (unsigned int g16 = 1; g16 <= 4200; ++g16)
        for (unsigned int resident : {4u, 1024u})
            for (int occ = 1; occ <= 2; ++occ)
                for (int knobs = 0; knobs < 6; ++knobs, ++n) {
                    mm_knob ko, kw;
                    ko.set = knobs & 1, ko.value = 2;
                    kw.set = knobs >= 2, kw.value = knobs >= 4 ? 0 : 3;
                    const mm_nuts_lgq_shape s = mm_nuts_lgq_grid(g16, resident, occ, ko, kw);
                    CHECK(s.occ == 1 || s.occ == 2, "g16 %u resident %u: occ %d", g16, resident, s.occ);
                    const unsigned int cap = g16 < resident * (unsigned int)s.occ ? g16 : resident * (unsigned int)s.occ;
                    CHECK(s.nw >= 1 && s.nw <= cap, "g16 %u resident %u occ %d knobs %d: %u waves, at most %u", g16, resident, occ, knobs, s.nw, cap);
                    CHECK(g16 >= 2 * resident || s.occ == 1, "g16 %u resident %u: two waves per SIMD cannot be filled", g16, resident);
                    const int asked = ko.set ? 2 : occ;
                    CHECK(g16 < 2 * resident || s.occ == asked, "g16 %u resident %u: occ %d, asked %d", g16, resident, s.occ, asked);
                    if (!kw.set || kw.value == 0)
                        CHECK(s.nw == cap, "g16 %u resident %u: %u waves without a knob, not %u", g16, resident, s.nw, cap);
                    else
                        CHECK(s.nw == (cap < 3u ? cap : 3u), "g16 %u resident %u: %u waves under the knob", g16, resident, s.nw);
                }
    /* the level: unknown below 8 transitions per chain; the mode minus one within [3, max_depth] */
    const size_t chains = 100;
    for (int mode = 0; mode <= MM_NUTS_JMAX; ++mode)
        for (int max_depth : {2, 5, 10, 12}) {
            ++n;
            unsigned int h[MM_NUTS_JMAX + 1] = {};
            h[mode] = 500;
            h[(mode + 1) % (MM_NUTS_JMAX + 1)] = 299; /* 799 counts: one short */
            CHECK(mm_nuts_level_from_hist(h, chains, max_depth) == -1, "mode %d: a level from 799 counts of 100 chains", mode);
            h[(mode + 2) % (MM_NUTS_JMAX + 1)] = 1; /* 800 */
            int want = mode - 1 < 3 ? 3 : mode - 1;
            want = want < max_depth ? want : max_depth;
            const int got = mm_nuts_level_from_hist(h, chains, max_depth);
            CHECK(got == want, "mode %d max_depth %d: level %d, not %d", mode, max_depth, got, want);
        }
    unsigned int tie[MM_NUTS_JMAX + 1] = {};
    tie[6] = tie[9] = 400; /* a tie goes to the shallower depth */
    CHECK(mm_nuts_level_from_hist(tie, chains, 10) == 5, "tie");
    CHECK(mm_nuts_lgq_pilot == 16u && mm_nuts_lgq_patience == 1u && mm_nuts_lgq_min_unit == 16u, "the measured constants");
    return n;
}

static long g_splits = 0;
static long pilots()
{
    long n = 0;
    const unsigned int pilot = 16, m0 = 7;
    for (unsigned int n_pre = 0; n_pre <= 40; ++n_pre)
        for (unsigned int n_rec = 0; n_rec <= 80; ++n_rec)
            for (unsigned int wi = 0; wi <= 1; ++wi)
                for (unsigned int t0 : {0u, 3u})
                    for (int known = 0; known < 2; ++known, ++n) {
                        const mm_nuts_segment a = {m0, n_pre, n_rec, wi, t0};
                        const mm_nuts_pilot_plan p = mm_nuts_pilot_split(a, known != 0, pilot);
                        const unsigned int total = n_pre + n_rec;
                        if (known || total < 4 * pilot) {
                            const mm_nuts_segment &s = p.seg[0];
                            CHECK(p.n == 1 && s.m0 == a.m0 && s.n_pre == a.n_pre && s.n_rec == a.n_rec && s.write_initial == a.write_initial &&
                                      s.out_t0 == a.out_t0,
                                  "pre %u rec %u known %d: split or changed", n_pre, n_rec, known);
                            continue;
                        }
                        ++g_splits;
                        CHECK(p.n == 2, "pre %u rec %u: no split", n_pre, n_rec);
                        const mm_nuts_segment &s1 = p.seg[0], &s2 = p.seg[1];
                        CHECK(s1.m0 == m0 && s1.n_pre + s1.n_rec == pilot && s2.m0 == m0 + pilot, "pre %u rec %u: the pilot is %u + %u from %u, the rest from %u",
                              n_pre, n_rec, s1.n_pre, s1.n_rec, s1.m0, s2.m0);
                        CHECK(s1.n_pre + s2.n_pre == n_pre && s1.n_rec + s2.n_rec == n_rec, "pre %u rec %u: %u + %u, %u + %u", n_pre, n_rec, s1.n_pre,
                              s2.n_pre, s1.n_rec, s2.n_rec);
                        /* in order: nothing is recorded before the last unrecorded transition */
                        CHECK(s1.n_rec == 0 || s2.n_pre == 0, "pre %u rec %u: recorded in the pilot, unrecorded after it", n_pre, n_rec);
                        CHECK(s1.write_initial == wi && s2.write_initial == 0u, "pre %u rec %u wi %u: initial row %u / %u", n_pre, n_rec, wi,
                              s1.write_initial, s2.write_initial);
                        /* rows: the one launch writes [t0, t0 + wi + n_rec); the pilot the first wi + s1.n_rec of them, the rest follows */
                        CHECK(s1.out_t0 == t0 && s2.out_t0 == t0 + wi + s1.n_rec, "pre %u rec %u wi %u: rows from %u and %u", n_pre, n_rec, wi, s1.out_t0,
                              s2.out_t0);
                        CHECK(s2.out_t0 + s2.n_rec == t0 + wi + n_rec, "pre %u rec %u wi %u: the rows end at %u", n_pre, n_rec, wi, s2.out_t0 + s2.n_rec);
                    }
    return n;
}

static long g_groups = 0, g_transitions = 0;
static void groups_of(size_t chains, long *n)
{
    const size_t c_pad = (chains + 15) / 16 * 16, waves = c_pad / 16;
    for (int req = 0; req <= 16; ++req, ++*n) {
        const int ng = mm_nuts_lg_n_groups(req, chains, c_pad);
        const size_t cap = waves < MM_NUTS_LG_MAX_GROUPS ? waves : MM_NUTS_LG_MAX_GROUPS;
        CHECK(ng >= 1 && (size_t)ng <= cap, "chains %zu requested %d: %d groups", chains, req, ng);
        if (req > 0)
            CHECK((size_t)ng == ((size_t)req < cap ? (size_t)req : cap), "chains %zu requested %d: %d groups", chains, req, ng);
        else
            CHECK((size_t)ng == (chains / 16384 < 1 ? 1 : chains / 16384 < cap ? chains / 16384 : cap), "chains %zu: %d groups by default", chains, ng);
        size_t next_w = 0, sum = 0;
        for (int gi = 0; gi < ng; ++gi, ++g_groups) {
            const mm_nuts_lg_group q = mm_nuts_lg_group_of(gi, ng, chains, c_pad);
            CHECK(q.w0 == next_w && q.w1 > q.w0, "chains %zu groups %d: group %d is waves [%zu, %zu) after %zu", chains, ng, gi, q.w0, q.w1, next_w);
            CHECK(q.offset == q.w0 * 16 && q.c_pad == (q.w1 - q.w0) * 16 && q.c_pad % 16 == 0, "chains %zu groups %d group %d: offset %zu c_pad %zu", chains,
                  ng, gi, q.offset, q.c_pad);
            CHECK(q.n_chains >= 1 && q.n_chains <= q.c_pad && q.c_pad - q.n_chains < 16, "chains %zu groups %d group %d: %zu chains in %zu slots", chains, ng, gi,
                  q.n_chains, q.c_pad);
            CHECK(gi == ng - 1 || q.n_chains == q.c_pad, "chains %zu groups %d group %d: padding inside the run", chains, ng, gi);
            next_w = q.w1;
            sum += q.n_chains;
        }
        CHECK(next_w == waves && sum == chains, "chains %zu groups %d: %zu waves, %zu chains covered", chains, ng, next_w, sum);
    }
}
static long groups()
{
    long n = 0;
    for (size_t chains = 1; chains <= 700; ++chains)
        groups_of(chains, &n);
    for (size_t chains : {(size_t)2048, (size_t)32768, (size_t)65535})
        groups_of(chains, &n);
    /* every transition's step and row, against the one-launch kernel: step m0 + t + 1; the initial row with the first
     * transition only; recorded transition r = t - n_pre goes to row out_t0 + write_initial + r */
    for (unsigned int n_pre = 0; n_pre <= 5; ++n_pre)
        for (unsigned int n_rec = 0; n_rec <= 5; ++n_rec)
            for (unsigned int wi = 0; wi <= 1; ++wi)
                for (unsigned int t0 : {0u, 3u}) {
                    const mm_nuts_segment a = {11u, n_pre, n_rec, wi, t0};
                    unsigned int next_row = t0 + wi;
                    for (unsigned int t = 0; t < n_pre + n_rec; ++t, ++g_transitions) {
                        const mm_nuts_lg_step s = mm_nuts_lg_step_of(a, t);
                        CHECK(s.m == 12u + t, "t %u: step %u", t, s.m);
                        CHECK(s.write_initial == (t == 0 ? wi : 0u), "t %u wi %u: %u", t, wi, s.write_initial);
                        CHECK((s.row == 0xffffffffu) == (t < n_pre), "pre %u t %u: row %u", n_pre, t, s.row);
                        if (t >= n_pre)
                            CHECK(s.row == next_row++, "pre %u rec %u wi %u t %u: row %u", n_pre, n_rec, wi, t, s.row);
                    }
                    CHECK(next_row == t0 + wi + n_rec, "pre %u rec %u: rows end at %u", n_pre, n_rec, next_row);
                }
    return n;
}

int main()
{
    const long s = steps(), p = paths(), c = schedules(), q = pilots(), g = groups();
    std::printf("step plans %ld caps %ld handles %ld accepted %ld schedules %ld pilot cases %ld splits %ld group cases %ld groups %ld transitions %ld failed %ld\n",
                s, p, g_handles, g_accepted, c, q, g_splits, g, g_groups, g_transitions, g_failed);
    return g_failed ? 1 : 0;
}
