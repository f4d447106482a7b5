/* The rules of the run-time compiled units (csrc/mm_rtc_units.h) on the host; a stand-alone program, built with the sanitizers
 * by tests/test_rtc_units_host.py.
 *
 *     rtc_units <functor dir> <out dir>
 *
 * A. texts: every case of tests/golden/rtc_unit_texts.json from the builders, one file <out dir>/<case>.hip each (the Python
 *    test compares length, sha256 and kernel names with the record taken from the parent commit).
 * B. the kernel table of every unit kind at dims 1, 8, 9, 32, literally; and per text of A: every table entry is a kernel
 *    the text emits, every emitted kernel is in the table -- but for the built-in MH / HMC unit's mmu_mh_split_f32.
 * C. the child-result rule over spawned x reaped elsewhere x {exit 0, 1, 2, 126, 127, a signal, the time-out's -1} x
 *    {code object present, empty, absent}; the environment filter over every dropped prefix and near misses.
 * D. the unit-kind predicates, for every kind.
 * Prints how many cases it walked; the counts are asserted in the Python test. */
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <set>
#include <sstream>

#include "../../mini_mcmc_amd/csrc/mm_rtc_units.h"

static int g_failed = 0;
#define CHECK(cond, ...)                                                                                                               \
    do {                                                                                                                               \
        if (!(cond)) {                                                                                                                 \
            ++g_failed;                                                                                                                \
            std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond);                                                               \
            std::printf(__VA_ARGS__);                                                                                                  \
            std::printf("\n");                                                                                                         \
        }                                                                                                                              \
    } while (0)

static std::string read_text(const std::string &path)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) {
        std::printf("cannot read %s\n", path.c_str());
        std::exit(2);
    }
    std::stringstream s;
    s << f.rdbuf();
    return s.str();
}

/* the names of the extern "C" kernels of a text, in order */
static std::vector<std::string> emitted_kernels(const std::string &text)
{
    std::vector<std::string> names;
    const std::string mark = "extern \"C\" __global__ ";
    for (size_t at = text.find(mark); at != std::string::npos; at = text.find(mark, at + 1)) {
        const size_t v = text.find("void ", at), open = text.find('(', v);
        names.push_back(text.substr(v + 5, open - v - 5));
    }
    return names;
}

static std::string table_text(mm_unit_kind k, int dim)
{
    std::string s;
    for (const mm_unit_kernel &e : mm_unit_kernels(k, dim)) {
        const std::string i = "[" + std::to_string(e.i) + "]", j = "[" + std::to_string(e.j) + "]";
        s += e.name + " " +
             (e.slot == MM_SLOT_RUN ? "run" + i + j : e.slot == MM_SLOT_LG ? "lg" + i : e.slot == MM_SLOT_NUTS ? "nuts" + i + j : e.slot == MM_SLOT_SPLIT ? "split" + i : std::string("disc")) +
             (e.required ? " req\n" : " opt\n");
    }
    return s;
}

/* ---- B: the tables, literally ------------------------------------------------------------------------------------------ */
#define NUTS_ROWS(infix, which, row, need)                                                                                               \
    "mmu_nuts_" infix which "_m0 nuts[" row "][0] " need "\nmmu_nuts_" infix which "_m1 nuts[" row "][1] " need "\nmmu_nuts_" infix which      \
    "_m2 nuts[" row "][2] " need "\n"
static const char *const kMh = "mmu_mh_f32 run[0][0] req\nmmu_mh_f64 run[0][1] req\n";
static const char *const kHmc = "mmu_hmc_f32 run[1][0] req\nmmu_hmc_f64 run[1][1] req\n";
static const char *const kLg = "mmu_logp_grad_f32 lg[0] req\nmmu_logp_grad_f64 lg[1] req\n";
static const char *const kPlainNuts = NUTS_ROWS("", "init", "0", "req") NUTS_ROWS("", "run", "1", "req") NUTS_ROWS("", "pair", "2", "opt");
static const char *const kMetric = "mmu_hmc_metric_f32 run[1][0] req\nmmu_hmc_metric_f64 run[1][1] req\n" NUTS_ROWS("metric_", "init", "0", "req")
    NUTS_ROWS("metric_", "run", "1", "req") NUTS_ROWS("metric_", "pair", "2", "req");
static const char *const kStats = NUTS_ROWS("stats_", "init", "0", "req") NUTS_ROWS("stats_", "run", "1", "req") NUTS_ROWS("stats_", "pair", "2", "req");
static const char *const kSplitMh = "mmu_mh_split_f32 split[0] opt\n";
static const char *const kSplitHmc = "mmu_hmc_split_f32 split[1] opt\nmmu_hmc_split_l10_f32 split[2] opt\n";

static std::string expected_table(mm_unit_kind k, int dim)
{
    const bool small = dim <= 8;
    switch (k) {
    case MM_RTC_UNIT_DISCRETE:
        return "mmu_discrete disc req\n";
    case MM_RTC_UNIT_METRIC:
        return kMetric;
    case MM_RTC_UNIT_STATS:
        return kStats;
    case MM_RTC_UNIT_BUILTIN_NUTS:
        return kPlainNuts;
    case MM_RTC_UNIT_MODEL:
        return std::string(kMh) + (small ? kSplitMh : "");
    case MM_RTC_UNIT_BUILTIN:
        return std::string(kMh) + kHmc; /* no lg, NUTS or split */
    case MM_RTC_UNIT_TARGET:
        return std::string(kMh) + kHmc + kLg + kPlainNuts + (small ? std::string(kSplitMh) + kSplitHmc : std::string());
    default:
        return "?";
    }
}

static int walk_tables()
{
    int n = 0;
    for (int k = 0; k < MM_RTC_UNIT_KINDS; ++k)
        for (int dim : {1, 8, 9, 32}) {
            const std::string got = table_text((mm_unit_kind)k, dim), want = expected_table((mm_unit_kind)k, dim);
            CHECK(got == want, "unit kind %d dim %d:\n%s-- expected\n%s", k, dim, got.c_str(), want.c_str());
            ++n;
        }
    return n;
}

/* ---- A: the texts, and B's cross-check ---------------------------------------------------------------------------------- */
static int g_texts = 0, g_crossed = 0;
static void emit(const std::string &out_dir, const std::string &name, mm_unit_kind k, int dim, const std::string &text)
{
    std::ofstream f(out_dir + "/" + name + ".hip", std::ios::binary);
    f << text;
    f.close();
    CHECK(f.good(), "writing %s", name.c_str());
    ++g_texts;
    const std::vector<std::string> emitted = emitted_kernels(text);
    const std::set<std::string> in_text(emitted.begin(), emitted.end());
    CHECK(in_text.size() == emitted.size(), "%s emits a kernel twice", name.c_str());
    std::set<std::string> in_table;
    for (const mm_unit_kernel &e : mm_unit_kernels(k, dim)) {
        in_table.insert(e.name);
        CHECK(in_text.count(e.name) == 1, "%s: the table's %s is not in the text", name.c_str(), e.name.c_str());
    }
    for (const std::string &e : emitted) {
        /* the one exception: the built-in MH / HMC unit's text holds the split MH kernel under MM_USER_DIM <= 8, dimensions that
         * never reach it; the loader does not ask for it */
        const bool exception = k == MM_RTC_UNIT_BUILTIN && e == "mmu_mh_split_f32";
        CHECK((in_table.count(e) == 1) != exception, "%s: the text's %s and the table disagree", name.c_str(), e.c_str());
    }
    ++g_crossed;
}

static void walk_texts(const std::string &in, const std::string &out)
{
    const std::string banana = read_text(in + "/banana.txt"), banana_logp = mm_unit_functor_logp(read_text(in + "/banana_logp.txt")),
                      linreg3_hand = mm_unit_functor_data(read_text(in + "/linreg3_hand.txt"), MMCMC_SOURCE_LOGP_GRAD),
                      linreg3_logp = mm_unit_functor_data(read_text(in + "/linreg3_logp.txt"), MMCMC_SOURCE_LOGP),
                      isotropic = read_text(in + "/isotropic.txt"), poisson = read_text(in + "/poisson_reflect.txt");
    const int user = MMCMC_USER_KIND_BASE; /* any caller's kind: its number is not part of a text */
    emit(out, "target_banana", MM_RTC_UNIT_TARGET, 2, mm_unit_text_target(banana, 2));
    emit(out, "target_banana_logp", MM_RTC_UNIT_TARGET, 2, mm_unit_text_target(banana_logp, 2));
    emit(out, "target_linreg3_hand", MM_RTC_UNIT_TARGET, 3, mm_unit_text_target(linreg3_hand, 3));
    emit(out, "target_linreg3_logp", MM_RTC_UNIT_TARGET, 3, mm_unit_text_target(linreg3_logp, 3));
    emit(out, "model_gaussian2d", MM_RTC_UNIT_MODEL, 2, mm_unit_text_model("", MMCMC_GAUSSIAN2D, isotropic));
    emit(out, "model_banana", MM_RTC_UNIT_MODEL, 2, mm_unit_text_model(banana, user, isotropic));
    emit(out, "model_linreg3", MM_RTC_UNIT_MODEL, 3, mm_unit_text_model(linreg3_hand, user + 2, isotropic));
    emit(out, "discrete_poisson_reflect", MM_RTC_UNIT_DISCRETE, 1, mm_unit_text_discrete(poisson));
    for (int dim : {9, 16, 17})
        emit(out, "builtin_rosenbrock_" + std::to_string(dim), MM_RTC_UNIT_BUILTIN, dim, mm_unit_text_builtin(MMCMC_ROSENBROCK_ND, dim));
    emit(out, "builtin_nuts_rosenbrock_9", MM_RTC_UNIT_BUILTIN_NUTS, 9, mm_unit_text_builtin_nuts(MMCMC_ROSENBROCK_ND, 9));
    emit(out, "builtin_nuts_gaussian_17", MM_RTC_UNIT_BUILTIN_NUTS, 17, mm_unit_text_builtin_nuts(MMCMC_GAUSSIAN_ND, 17));
    const mm_unit_functor m_rosen = mm_unit_functor_of(MMCMC_ROSENBROCK_ND, "", "mmu_metric_target"), m_banana = mm_unit_functor_of(user, banana, "mmu_metric_target"),
                          m_linreg3 = mm_unit_functor_of(user + 2, linreg3_hand, "mmu_metric_target");
    for (int mk = 1; mk <= 2; ++mk) {
        const std::string word = mk == 2 ? "dense" : "metric";
        emit(out, word + "_rosenbrock_3", MM_RTC_UNIT_METRIC, 3, mm_unit_text_metric(m_rosen, 3, mk));
        emit(out, word + "_rosenbrock_17", MM_RTC_UNIT_METRIC, 17, mm_unit_text_metric(m_rosen, 17, mk));
        emit(out, word + "_banana", MM_RTC_UNIT_METRIC, 2, mm_unit_text_metric(m_banana, 2, mk));
    }
    emit(out, "metric_linreg3", MM_RTC_UNIT_METRIC, 3, mm_unit_text_metric(m_linreg3, 3, 1));
    const mm_unit_functor s_rosen = mm_unit_functor_of(MMCMC_ROSENBROCK_ND, "", "mmu_stats_target"), s_banana = mm_unit_functor_of(user, banana, "mmu_stats_target");
    for (int mk = 0; mk <= 2; ++mk) {
        emit(out, "stats" + std::to_string(mk) + "_rosenbrock_3", MM_RTC_UNIT_STATS, 3, mm_unit_text_stats(s_rosen, 3, mk));
        emit(out, "stats" + std::to_string(mk) + "_banana", MM_RTC_UNIT_STATS, 2, mm_unit_text_stats(s_banana, 2, mk));
    }
}

/* ---- C: the child rules -------------------------------------------------------------------------------------------------- */
static int walk_child_results()
{
    /* status as wait() encodes it: exit code << 8; low seven bits = the signal that killed it; -1: killed after the time-out */
    const int statuses[7] = {0 << 8, 1 << 8, 2 << 8, 126 << 8, 127 << 8, 9, -1};
    const long sizes[3] = {4096, 0, -1}; /* present, empty, absent */
    /* spawned and reaped here: [status][size] */
    const int ours[7][3] = {{0, 1, 1},  /* exit 0: the code object, or nothing to read */
                            {2, 2, 2},  /* exit 1: the compiler rejected the source */
                            {2, 2, 2},  /* exit 2 */
                            {1, 1, 1},  /* exit 126: the launcher could not run the compiler */
                            {1, 1, 1},  /* exit 127 */
                            {1, 1, 1},  /* a signal */
                            {1, 1, 1}}; /* the time-out */
    const int elsewhere[3] = {0, 2, 2}; /* reaped elsewhere: judged by the code object alone, whatever the status variable holds */
    int n = 0;
    for (int spawned = 0; spawned < 2; ++spawned)
        for (int reaped_elsewhere = 0; reaped_elsewhere < 2; ++reaped_elsewhere)
            for (int s = 0; s < 7; ++s)
                for (int z = 0; z < 3; ++z) {
                    const int want = !spawned ? 1 : reaped_elsewhere ? elsewhere[z] : ours[s][z];
                    const int got = mm_unit_child_result(spawned != 0, reaped_elsewhere != 0, statuses[s], sizes[z]);
                    CHECK(got == want, "spawned %d reaped elsewhere %d status %d size %ld: %d, expected %d", spawned, reaped_elsewhere, statuses[s], sizes[z], got, want);
                    ++n;
                }
    return n;
}

static int walk_env()
{
    struct Entry {
        const char *text;
        bool kept;
    };
    const Entry entries[] = {{"PATH=/usr/bin:/opt/rocm/bin", true},
                             {"LD_PRELOAD=/opt/tool/lib.so", false},
                             {"MY_LD_PRELOAD=x", true},
                             {"HSA_TOOLS_LIB=librocprofiler-sdk-tool.so", false},
                             {"HSA_TOOLS_REPORT_LOAD_FAILURE=1", false},
                             {"ROC_X=1", true},
                             {"ROCP_TOOL_LIBRARIES=x", false},
                             {"ROCPROFILER_LIBRARY_CTOR=1", false},
                             {"ROCPROF=1", false},
                             {"HOME=/home/u", true},
                             {"ROCTRACER_DOMAIN=hip", false},
                             {"ROCTX_X=", false},
                             {"HIP_TOOLS_LIB=x", false},
                             {"LD_AUDIT=x", false},
                             {"LD_PRELOAD=", false},
                             {"LD_PRELOAD", true},  /* no '=': another variable's name begins so */
                             {"HIP_TOOLS_LIBX=x", true},
                             {"ROCM_PATH=/opt/rocm", true},
                             {"", true},
                             {"TMPDIR=/tmp", true}};
    std::vector<char *> env, want;
    std::vector<std::string> store;
    for (const Entry &e : entries)
        store.push_back(e.text);
    for (size_t i = 0; i < store.size(); ++i) {
        env.push_back(&store[i][0]);
        if (entries[i].kept)
            want.push_back(&store[i][0]);
    }
    env.push_back(nullptr);
    const std::vector<char *> got = mm_unit_child_env(env.data());
    CHECK(got == want, "kept %zu entries, expected %zu (the same pointers, in order)", got.size(), want.size());
    char *none[] = {nullptr};
    CHECK(mm_unit_child_env(none).empty() && mm_unit_child_env(nullptr).empty(), "an empty environment");
    return (int)store.size();
}

/* ---- D: the predicates ---------------------------------------------------------------------------------------------------- */
static int walk_predicates()
{
    struct Row {
        mm_unit_kind k;
        bool model, discrete, internal, functor;
    };
    const Row rows[] = {{MM_RTC_UNIT_TARGET, false, false, false, true},        {MM_RTC_UNIT_MODEL, true, false, false, false},
                        {MM_RTC_UNIT_DISCRETE, false, true, false, false},      {MM_RTC_UNIT_BUILTIN, false, false, true, false},
                        {MM_RTC_UNIT_BUILTIN_NUTS, false, false, true, false},  {MM_RTC_UNIT_METRIC, false, false, true, false},
                        {MM_RTC_UNIT_STATS, false, false, true, false}};
    int n = 0;
    CHECK(sizeof rows / sizeof rows[0] == MM_RTC_UNIT_KINDS, "a row per kind");
    for (const Row &r : rows) {
        CHECK(mm_unit_is_model(r.k) == r.model, "kind %d", (int)r.k);
        CHECK(mm_unit_is_discrete(r.k) == r.discrete, "kind %d", (int)r.k);
        CHECK(mm_unit_is_internal(r.k) == r.internal, "kind %d", (int)r.k);
        CHECK(mm_unit_carries_functor(r.k) == r.functor, "kind %d", (int)r.k);
        CHECK(!(r.model && mm_unit_carries_functor(r.k)), "a model is not a gradient target");
        n += 4;
    }
    return n;
}

static int walk_flags()
{
    const std::vector<std::string> f = mm_unit_compile_flags("gfx950:sramecc+:xnack-", 7);
    const std::vector<std::string> want = {"--offload-arch=gfx950:sramecc+:xnack-", "-O3", "-ffp-contract=off", "-std=c++17", "-DMM_USER_DIM=7", "-Wno-pass-failed"};
    CHECK(f == want, "the compile flags");
    return 1;
}

int main(int argc, char **argv)
{
    if (argc != 3) {
        std::printf("usage: %s <functor dir> <out dir>\n", argv[0]);
        return 2;
    }
    walk_texts(argv[1], argv[2]);
    const int tables = walk_tables(), results = walk_child_results(), env = walk_env(), predicates = walk_predicates(), flags = walk_flags();
    std::printf("texts %d tables %d crossed %d child results %d env entries %d predicates %d flag lists %d failed %d\n", g_texts, tables, g_crossed, results, env,
                predicates, flags, g_failed);
    return g_failed ? 1 : 0;
}
