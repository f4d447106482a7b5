/* mm_rtc_units.h -- the rules of the run-time compiled units (mm_rtc.hip), host-only and pure: the unit kinds and what each
 * kind is, the table of kernels a kind has (what the loader asks the module for), the text of each kind's unit, the compile
 * flags, and the two decisions around the compiler child (its environment, what its end means).  No HIP, no environment, no
 * globals: tests/cpp/rtc_units.cpp walks every rule here on the host, and tests/golden/rtc_unit_texts.json pins the texts. */
#ifndef MM_RTC_UNITS_H
#define MM_RTC_UNITS_H

#include <string>
#include <vector>

#include "../../include/mmcmc.h"

/* the NUTS pair kernel (asynchronous lanes, leaves in pairs) is compiled up to this dimension */
#define MM_RTC_NUTS_PAIR_MAX_DIM 32

/* ---- unit kinds ------------------------------------------------------------------------------------------------------- */
enum mm_unit_kind {
    MM_RTC_UNIT_TARGET = 0,   /* a caller's target (hand gradient, autodiff, data): MH, HMC, batch logp / gradient, NUTS */
    MM_RTC_UNIT_MODEL,        /* target + caller's proposal in one class (mmcmc_proposal_register_source): MH kernels only */
    MM_RTC_UNIT_DISCRETE,     /* an integer-state model (mmcmc_discrete_register_source): one kernel */
    MM_RTC_UNIT_BUILTIN,      /* a built-in target at a dimension without a compiled instance: MH + HMC */
    MM_RTC_UNIT_BUILTIN_NUTS, /* the same for NUTS */
    MM_RTC_UNIT_METRIC,       /* HMC and NUTS kernels that read a diagonal or a dense metric, around a target's functor */
    MM_RTC_UNIT_STATS,        /* NUTS kernels that record per-draw statistics, with no metric, a diagonal or a dense one */
    MM_RTC_UNIT_KINDS
};

static inline bool mm_unit_is_model(mm_unit_kind k) { return k == MM_RTC_UNIT_MODEL; }
static inline bool mm_unit_is_discrete(mm_unit_kind k) { return k == MM_RTC_UNIT_DISCRETE; }
/* a unit the library built for itself: not a kind a caller may name in a description */
static inline bool mm_unit_is_internal(mm_unit_kind k)
{
    return k == MM_RTC_UNIT_BUILTIN || k == MM_RTC_UNIT_BUILTIN_NUTS || k == MM_RTC_UNIT_METRIC || k == MM_RTC_UNIT_STATS;
}
/* the registered kind keeps the source of a gradient functor, mmcmc_user_target<T>: what a model, a metric unit and a stats
 * unit over a caller's kind are compiled around */
static inline bool mm_unit_carries_functor(mm_unit_kind k) { return k == MM_RTC_UNIT_TARGET; }

/* ---- kernel names ----------------------------------------------------------------------------------------------------- */
/* type modes of NUTS: 0 (f32 tensors, f64 scalars), 1 (f32, f32), 2 (f64, f64) */
static inline const char *mm_unit_nuts_type(int mode, int scalar)
{
    static const char *const types[3][2] = {{"float", "double"}, {"float", "float"}, {"double", "double"}};
    return types[mode][scalar];
}
/* mmu_{mh,hmc}_<infix>{f32,f64}: infix "" (a target's own kernels) or "metric_" */
static inline std::string mm_unit_run_name(int sampler, const std::string &infix, int dtype)
{
    return std::string(sampler ? "mmu_hmc_" : "mmu_mh_") + infix + (dtype ? "f64" : "f32");
}
static inline const char *mm_unit_lg_name(int dtype) { return dtype ? "mmu_logp_grad_f64" : "mmu_logp_grad_f32"; }
/* f32 MH / HMC / HMC with L = 10 unrolled on the four-waves-per-SIMD kernel */
static inline const char *mm_unit_split_name(int which)
{
    static const char *const names[3] = {"mmu_mh_split_f32", "mmu_hmc_split_f32", "mmu_hmc_split_l10_f32"};
    return names[which];
}
/* mmu_nuts_<infix>{init,run,pair}_m<mode>: infix "", "metric_" or "stats_"; which 0 init, 1 lanes in step, 2 pairs */
static inline std::string mm_unit_nuts_name(const std::string &infix, int which, int mode)
{
    static const char *const parts[3] = {"init", "run", "pair"};
    return "mmu_nuts_" + infix + parts[which] + "_m" + std::to_string(mode);
}
static inline const char *mm_unit_discrete_name() { return "mmu_discrete"; }

/* ---- the kernel table ------------------------------------------------------------------------------------------------- */
/* where the loader keeps a kernel: run[i][j] (sampler, dtype), lg[i] (dtype), nuts[i][j] (init / run / pair, mode), split[i], disc */
enum mm_unit_slot { MM_SLOT_RUN, MM_SLOT_LG, MM_SLOT_NUTS, MM_SLOT_SPLIT, MM_SLOT_DISC };
struct mm_unit_kernel {
    std::string name;
    mm_unit_slot slot;
    int i, j;
    bool required; /* missing: the load fails; an optional kernel that is missing leaves a null slot and another kernel runs */
};

/* The kernels the loader asks a unit's module for, in the order it asks.  A metric or a stats unit has every kernel or does
 * not load: a handle with a metric has no other kernel to fall back on.  Optional are the kernels with a slower twin of the
 * same bits: the NUTS pair kernel (the lanes-in-step kernel runs instead) and the four-waves-per-SIMD kernels of dim <= 8
 * (the one-wave kernel runs instead).  dim <= MM_RTC_NUTS_PAIR_MAX_DIM is always true today -- every entry enforces
 * dim <= 32 -- and stays as the documented limit.  Observed, not a rule: the built-in MH / HMC unit's text holds
 * mmu_mh_split_f32 under MM_USER_DIM <= 8, dimensions that have compiled instances and never reach it; the table does not
 * list that kernel and the loader never asks for it. */
static inline std::vector<mm_unit_kernel> mm_unit_kernels(mm_unit_kind k, int dim)
{
    std::vector<mm_unit_kernel> v;
    auto nuts = [&](const std::string &infix, int from, int to, bool required) {
        for (int i = from; i < to; ++i)
            for (int m = 0; m < 3; ++m)
                v.push_back({mm_unit_nuts_name(infix, i, m), MM_SLOT_NUTS, i, m, required});
    };
    auto plain_nuts = [&]() {
        nuts("", 0, 2, true);
        if (dim <= MM_RTC_NUTS_PAIR_MAX_DIM)
            nuts("", 2, 3, false);
    };
    switch (k) {
    case MM_RTC_UNIT_DISCRETE:
        v.push_back({mm_unit_discrete_name(), MM_SLOT_DISC, 0, 0, true});
        return v;
    case MM_RTC_UNIT_METRIC:
        for (int t = 0; t < 2; ++t)
            v.push_back({mm_unit_run_name(1, "metric_", t), MM_SLOT_RUN, 1, t, true});
        nuts("metric_", 0, 3, true);
        return v;
    case MM_RTC_UNIT_STATS:
        nuts("stats_", 0, 3, true);
        return v;
    case MM_RTC_UNIT_BUILTIN_NUTS:
        plain_nuts();
        return v;
    default:
        break;
    }
    for (int s = 0; s < (k == MM_RTC_UNIT_MODEL ? 1 : 2); ++s)
        for (int t = 0; t < 2; ++t)
            v.push_back({mm_unit_run_name(s, "", t), MM_SLOT_RUN, s, t, true});
    if (k == MM_RTC_UNIT_TARGET) {
        for (int t = 0; t < 2; ++t)
            v.push_back({mm_unit_lg_name(t), MM_SLOT_LG, t, 0, true});
        plain_nuts();
    }
    if (dim <= 8)
        for (int sm = 0; sm < (k == MM_RTC_UNIT_MODEL ? 1 : k == MM_RTC_UNIT_BUILTIN ? 0 : 3); ++sm)
            v.push_back({mm_unit_split_name(sm), MM_SLOT_SPLIT, sm, 0, false});
    return v;
}

/* ---- the texts -------------------------------------------------------------------------------------------------------- */
/* the head of one kernel; bounds 0: no __launch_bounds__ */
static inline std::string mm_unit_head(int bounds, const std::string &name)
{
    return "extern \"C\" __global__ " + (bounds ? "__launch_bounds__(" + std::to_string(bounds) + ") " : std::string()) + "void " + name;
}

/* the f32 / f64 pair of one-wave-per-SIMD MH or HMC kernels around `cls<T>`; word "": the target's own (mm_run_kernel_body),
 * "metric" / "dense": the HMC kernels of a metric unit (mm_run_<word>_body over mm_run_<word>_args) */
static inline std::string mm_unit_run_pair(int sampler, const std::string &cls, int pipe, const std::string &word)
{
    std::string src;
    for (int t = 0; t < 2; ++t) {
        const std::string ty = t ? "double" : "float";
        if (word.empty())
            src += mm_unit_head(256, mm_unit_run_name(sampler, "", t)) + "(const mm_run_args<" + ty + "> a) { mm_run_kernel_body<" + ty + ", " +
                   cls + "<" + ty + ">, " + (sampler ? "MM_SAMPLER_HMC" : "MM_SAMPLER_MH") + ", " + std::to_string(pipe) + ", 0>(a); }\n";
        else
            src += mm_unit_head(256, mm_unit_run_name(sampler, "metric_", t)) + "(const mm_run_" + word + "_args<" + ty + "> m) { mm_run_" + word +
                   "_body<" + ty + ", " + cls + "<" + ty + ">, " + std::to_string(pipe) + ">(m); }\n";
    }
    return src;
}

/* the MH kernels (one wave per SIMD f32 / f64; four waves per SIMD f32 up to dim 8) around class `cls<T>` */
static inline std::string mm_unit_mh_kernels(const std::string &cls, int pipe)
{
    std::string src = mm_unit_run_pair(0, cls, pipe, "");
    src += "#if MM_USER_DIM <= 8\n";
    src += mm_unit_head(1024, mm_unit_split_name(0)) + "(const mm_run_args<float> a) { mm_run_split_body<float, " + cls +
           "<float>, MM_SAMPLER_MH, 0, mm_split_mh_qp<float, MM_USER_DIM, MM_SPLIT_NOISE_WAVES>::value, MM_SPLIT_NOISE_WAVES, 0>(a); }\n";
    src += "#endif\n";
    return src;
}

/* NUTS, one chain per lane, around `cls<T>`: init_chain, the run with the lanes in step and the run with leaves in pairs,
 * for the three type modes.  metric_kind 0 none / 1 diagonal / 2 dense picks the argument blocks and bodies; `stats`: the
 * run kernels carry the recording policy (mm_nuts_stats_args over the block of that metric kind), init is that metric kind's */
static inline std::string mm_unit_nuts_triple(const std::string &cls, int dim, int metric_kind, bool stats)
{
    static const char *const words[3] = {"", "metric_", "dense_"};
    const std::string w = words[metric_kind], infix = stats ? "stats_" : metric_kind ? "metric_" : "";
    std::string src;
    for (int m = 0; m < 3; ++m) {
        const std::string tt = mm_unit_nuts_type(m, 0), st = mm_unit_nuts_type(m, 1), types = "<" + tt + ", " + st + ">",
                          inst = "<" + tt + ", " + st + ", " + cls + "<" + tt + ">>";
        if (metric_kind == 0)
            src += mm_unit_head(64, mm_unit_nuts_name(infix, 0, m)) + "(const mm_nuts_init_args" + types + " a) { mm_nuts_init_body" + inst +
                   "(a.P, a.state, a.adapt, a.n_chains, a.seed, a.chain_offset, a.eps_tol); }\n";
        else
            src += mm_unit_head(64, mm_unit_nuts_name(infix, 0, m)) + "(const mm_nuts_init_" + w + "args" + types + " m) { mm_nuts_init_" + w +
                   "body" + inst + "(m); }\n";
        for (int i = 1; i < 3; ++i) {
            const std::string head = mm_unit_head(64, mm_unit_nuts_name(infix, i, m)), body = i == 1 ? "run_" : "pair_";
            if (stats)
                src += head + "(const mm_nuts_stats_args<mm_nuts_" + w + "args" + types + "> s) { mm_nuts_" + body + "stats_body" + inst + "(s); }\n";
            else if (metric_kind)
                src += head + "(const mm_nuts_" + w + "args" + types + " m) { mm_nuts_" + body + w + "body" + inst + "(m); }\n";
            else if (i == 1 || dim <= MM_RTC_NUTS_PAIR_MAX_DIM)
                src += head + "(const mm_nuts_args" + types + " a) { mm_nuts_" + body + "body<" + tt + ", " + st + ", " + cls + "<" + tt + ">, false>(a); }\n";
        }
    }
    return src;
}

/* a built-in target under a name of the unit's own */
static inline std::string mm_unit_builtin_alias(const std::string &alias, int target_kind)
{
    return "template <class T> using " + alias + " = mm_target<T, " + std::to_string(target_kind) + ", MM_USER_DIM>;\n";
}
/* above 16 the paired / pipelined form of the one-wave kernels spills (mm_api.hip) */
static inline int mm_unit_pipe(int dim) { return dim > 16 ? 0 : 2; }

/* mmcmc_user_logp<T> -> mmcmc_user_target<T>: value by logp<T>, gradient by forward mode (mm_autodiff.h) */
static inline const char *mm_unit_autodiff_adapter()
{
    return "\ntemplate <class T> struct mmcmc_user_target {\n"
           "    static constexpr int dim = mmcmc_user_logp<T>::dim;\n"
           "    MM_HD static T logp(const mm_tparams<T> &P, const T *x) { return mmcmc_user_logp<T>::template logp<T>(P, x); }\n"
           "    MM_HD static T logp_grad(const mm_tparams<T> &P, const T *x, T *g) { return mm_ad_logp_grad<T, mmcmc_user_logp<T>>(P, x, g); }\n"
           "};\n";
}
/* the functor text a caller's kind keeps, from what was registered.  A log-density alone (mmcmc_user_logp<T>) gets the adapter
 * appended, so a model, a metric or a stats unit over the kind compiles; a data kind gets the row helper in front, which
 * brings mm_autodiff.h (mm_softplusT, mm_sigmoidT) */
static inline std::string mm_unit_functor_logp(const std::string &source) { return "#include \"mm_autodiff.h\"\n" + source + mm_unit_autodiff_adapter(); }
static inline std::string mm_unit_functor_data(const std::string &source, int flavour)
{
    return "#include \"mm_data.h\"\n" + source + (flavour == MMCMC_SOURCE_LOGP ? mm_unit_autodiff_adapter() : "");
}

/* a caller's target: `functor` defines mmcmc_user_target<T>.  The MH / HMC kernels for f32 and f64 (dim <= 8: also on the
 * four-waves-per-SIMD kernel, three noise waves per transition wave), the batch log-density / gradient kernels, and NUTS
 * (GradientTarget is what nuts.rs:123-129 takes) with the stack in HBM */
static inline std::string mm_unit_text_target(const std::string &functor, int dim)
{
    const std::string cls = "mmcmc_user_target";
    std::string src = "#include \"mm_kernels.h\"\n#include \"mm_split_kernels.h\"\n#include \"mm_nuts_kernels.h\"\n";
    src += functor;
    src += "\nstatic_assert(mmcmc_user_target<float>::dim == MM_USER_DIM && mmcmc_user_target<double>::dim == MM_USER_DIM,"
           " \"mmcmc_user_target<T>::dim must equal the registered dimension\");\n";
    src += mm_unit_mh_kernels(cls, 2);
    src += mm_unit_run_pair(1, cls, 2, "");
    src += "#if MM_USER_DIM <= 8\n";
    for (int l10 = 0; l10 < 2; ++l10)
        src += mm_unit_head(1024, mm_unit_split_name(1 + l10)) + "(const mm_run_args<float> a) { mm_run_split_body<float, mmcmc_user_target<float>, MM_SAMPLER_HMC, " +
               (l10 ? "10" : "0") + ", 0, MM_SPLIT_NOISE_WAVES, 0>(a); }\n";
    src += "#endif\n";
    for (int t = 0; t < 2; ++t) {
        const std::string ty = t ? "double" : "float";
        src += mm_unit_head(0, mm_unit_lg_name(t)) + "(const mm_tparams<" + ty + "> P, const " + ty + " *x, " + ty + " *logp, " + ty +
               " *grad, unsigned long long n) {\n"
               "    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;\n"
               "    if (i >= n) return;\n"
               "    " + ty + " xv[MM_USER_DIM], gv[MM_USER_DIM];\n"
               "    for (int k = 0; k < MM_USER_DIM; ++k) xv[k] = x[i * MM_USER_DIM + k];\n"
               "    if (grad) { logp[i] = mmcmc_user_target<" + ty + ">::logp_grad(P, xv, gv); for (int k = 0; k < MM_USER_DIM; ++k) grad[i * MM_USER_DIM + k] = gv[k]; }\n"
               "    else logp[i] = mmcmc_user_target<" + ty + ">::logp(P, xv);\n}\n";
    }
    src += mm_unit_nuts_triple(cls, dim, 0, false);
    return src;
}

/* a model: the target's log-density plus `typedef mmcmc_user_proposal<T> proposal;`, the MH skeletons around it.
 * base_functor: the stored functor of a caller's kind, or "" for the built-in target_kind */
static inline std::string mm_unit_text_model(const std::string &base_functor, int target_kind, const std::string &proposal_source)
{
    std::string src = "#include \"mm_kernels.h\"\n#include \"mm_split_kernels.h\"\n";
    if (target_kind >= MMCMC_USER_KIND_BASE)
        src += base_functor + "\ntemplate <class T> using mmu_base = mmcmc_user_target<T>;\n";
    else
        src += mm_unit_builtin_alias("mmu_base", target_kind);
    src += proposal_source;
    src += "\ntemplate <class T> struct mmu_model : mmu_base<T> { typedef mmcmc_user_proposal<T> proposal; };\n"
           "static_assert(mmu_model<float>::dim == MM_USER_DIM, \"the target's dimension must equal the registered dimension\");\n";
    src += mm_unit_mh_kernels("mmu_model", 2);
    return src;
}

static inline std::string mm_unit_text_discrete(const std::string &source)
{
    return "#include \"mm_discrete_kernels.h\"\n" + source + "\n" + mm_unit_head(64, mm_unit_discrete_name()) +
           "(const mm_discrete_user_args a) { mm_discrete_user_body<mmcmc_user_discrete>(a); }\n";
}

/* a built-in target's MH / HMC kernels (mm_unit_mh_kernels also emits the four-waves-per-SIMD MH kernel for dim <= 8: those
 * dimensions have compiled instances and never come here, but the unit must build) */
static inline std::string mm_unit_text_builtin(int target_kind, int dim)
{
    return "#include \"mm_kernels.h\"\n" + mm_unit_builtin_alias("mmu_builtin", target_kind) + mm_unit_mh_kernels("mmu_builtin", mm_unit_pipe(dim)) +
           mm_unit_run_pair(1, "mmu_builtin", mm_unit_pipe(dim), "");
}
static inline std::string mm_unit_text_builtin_nuts(int target_kind, int dim)
{
    return "#include \"mm_kernels.h\"\n#include \"mm_nuts_kernels.h\"\n" + mm_unit_builtin_alias("mmu_builtin", target_kind) +
           mm_unit_nuts_triple("mmu_builtin", dim, 0, false);
}

/* what a metric or a stats unit is compiled around: the stored functor of a caller's kind (class mmcmc_user_target), or a
 * built-in target under `alias` */
struct mm_unit_functor {
    std::string text, cls;
};
static inline mm_unit_functor mm_unit_functor_of(int target_kind, const std::string &stored_functor, const std::string &alias)
{
    if (target_kind >= MMCMC_USER_KIND_BASE)
        return {stored_functor, "mmcmc_user_target"};
    return {mm_unit_builtin_alias(alias, target_kind), alias};
}
static inline std::string mm_unit_gradient_unit_head(const mm_unit_functor &f)
{
    return "#include \"mm_kernels.h\"\n#include \"mm_nuts_kernels.h\"\n" + f.text + "\nstatic_assert(" + f.cls + "<float>::dim == MM_USER_DIM && " + f.cls +
           "<double>::dim == MM_USER_DIM, \"the target's dimension must equal the handle's\");\n";
}
/* metric_kind 1 diagonal (mm_*_metric_*), 2 dense (mm_*_dense_*) */
static inline std::string mm_unit_text_metric(const mm_unit_functor &f, int dim, int metric_kind)
{
    return mm_unit_gradient_unit_head(f) + mm_unit_run_pair(1, f.cls, mm_unit_pipe(dim), metric_kind == 2 ? "dense" : "metric") +
           mm_unit_nuts_triple(f.cls, dim, metric_kind, false);
}
/* metric_kind 0 none, 1 diagonal, 2 dense */
static inline std::string mm_unit_text_stats(const mm_unit_functor &f, int dim, int metric_kind)
{
    return mm_unit_gradient_unit_head(f) + mm_unit_nuts_triple(f.cls, dim, metric_kind, true);
}

/* ---- the compiler ----------------------------------------------------------------------------------------------------- */
/* the flags of the library build (Makefile): -ffp-contract=off keeps a host restatement of the functor bit-exact.  The
 * `hipcc --genco` child gets them between "--genco" and its paths, hipRTC gets exactly them */
static inline std::vector<std::string> mm_unit_compile_flags(const std::string &arch, int dim)
{
    return {"--offload-arch=" + arch, "-O3", "-ffp-contract=off", "-std=c++17", "-DMM_USER_DIM=" + std::to_string(dim), "-Wno-pass-failed"};
}

/* The child's environment is the parent's MINUS everything that makes a tool library load into it: under rocprofv3
 * (LD_PRELOAD / HSA_TOOLS_LIB / ROCP_* ...) the profiler's library initialises the GPU at process start, and hipcc is a
 * launcher that execs clang, lld and the bundler -- an exec inside a GPU-initialised process, which shared machines forbid
 * (and which would pollute the profile).  The compiler needs none of them.  The kept entries, in their order. */
static inline std::vector<char *> mm_unit_child_env(char *const *env)
{
    static const char *const drop[] = {"LD_PRELOAD=", "HSA_TOOLS_LIB=", "HSA_TOOLS_REPORT_LOAD_FAILURE=", "ROCP_", "ROCPROF", "ROCTRACER_",
                                       "ROCTX_", "HIP_TOOLS_LIB=", "LD_AUDIT="};
    std::vector<char *> kept;
    for (char *const *e = env; e && *e; ++e) {
        bool keep = true;
        for (const char *d : drop) {
            size_t n = 0;
            while (d[n] && (*e)[n] == d[n])
                ++n;
            keep = keep && d[n] != 0;
        }
        if (keep)
            kept.push_back(*e);
    }
    return kept;
}

/* What the end of the compiler child means: 0 the code object is there to be read, 1 the compiler is not available or could
 * not be run (the caller may fall back to hipRTC), 2 it ran and rejected the source.  status: as wait() encodes it, or -1
 * after the time-out; code_size: bytes of the code object it left, < 0 if there is none.  A child reaped elsewhere (the host
 * ignores SIGCHLD or reaps children itself) has exited and its status is gone: it is judged by the code object.  Exit 126 /
 * 127 (the launcher could not run the compiler), a signal and the time-out all say "not available". */
static inline int mm_unit_child_result(bool spawned, bool reaped_elsewhere, int status, long code_size)
{
    if (reaped_elsewhere)
        status = code_size > 0 ? 0 : (1 << 8); /* exit 0 / exit 1 as wait() would encode them */
    const bool exited = (status & 0x7f) == 0; /* WIFEXITED / WEXITSTATUS: mm_rtc.hip asserts the encoding */
    const int code = (status >> 8) & 0xff;
    if (spawned && exited && code == 0)
        return code_size > 0 ? 0 : 1;
    if (spawned && exited && code != 127 && code != 126)
        return 2;
    return 1;
}

#endif /* MM_RTC_UNITS_H */
