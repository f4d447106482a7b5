/* stats_launch_trace.cpp -- the launches the diagnostics dispatch (csrc/mm_stats.hip) makes, recorded without a GPU.
 *
 * The unit itself is included below, after the HIP calls its host code makes have been redefined as recording stubs: what is
 * traced is the library's own dispatch, not a twin.  Pointers are fakes that nothing dereferences (the host code only does
 * arithmetic on them); the kernels are compiled and never run.
 *
 * One call = one line "call ...", one line per launch (kernel instance with its template arguments, grid, block, dynamic LDS
 * bytes, every argument: integers and floats by value, pointers as region+offset -- the workspace in floats, the others in
 * bytes), lines for a raised LDS limit and a table upload, and one line "ret" with the status, whether the path wrote the
 * total itself, the workspace size the sizing function gives and the bytes a call without a workspace allocates.
 *
 * The walk: 6 selectors x f32/f64 x aligned/unaligned sample x with/without wb_part x kM half-chain lengths x n in {2 m,
 * 2 m + 1} x kD dimensions x kC chain counts, then the direct-work limit at its default and at 0, then the two public
 * entry points' early statuses.  Usage:
 *    stats_launch_trace            one SHA-256 per m over that m's lines, "entry <sha>", "calls <count>"
 *    stats_launch_trace --lines M  the lines of half-chain length M (M = entry: the entry points' lines)
 *    stats_launch_trace --named    the lines of the named cases
 * -DSTATS_TRACE_PARENT: the internal function as it was before the plan header existed (to record the golden file). */
#include <hip/hip_runtime.h>

#include "../../mini_mcmc_amd/csrc/mm_host.h"

#include <cinttypes>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cxxabi.h>
#include <string>
#include <typeinfo>
#include <type_traits>
#include <utility>
#include <vector>

namespace trace {

/* fake address regions: [region << 40, (region + 1) << 40) below kWs, the workspace above it */
enum { R_SAMPLE = 0x10, R_MEANS, R_SSQ, R_ACOV, R_WB, R_FINAL, R_TABLE = 0x20 };
constexpr uintptr_t kWs = (uintptr_t)0x4000 << 32;
static void *region(unsigned int r, size_t off = 0) { return (void *)(((uintptr_t)r << 40) + off); }

static std::string g_lines;   /* of the call being traced */
static int g_dev_status = 0;  /* what mm_check_device answers */
static size_t g_alloc = 0;    /* bytes of the call's stream-ordered allocation */
static std::vector<size_t> g_tables; /* bytes of every table uploaded so far: region R_TABLE + index */

static void add(const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_lines += buf;
}

static void add_ptr(const void *p)
{
    const uintptr_t a = (uintptr_t)p;
    static const char *names[] = {"sample", "means", "ssq", "acov", "wb", "final"};
    if (!p)
        add(" null");
    else if (a >= kWs)
        add(" ws+%zu%s", (size_t)(a - kWs) / 4, (a - kWs) % 4 ? "?" : "");
    else if ((a >> 40) >= R_TABLE)
        add(" tab%zu+%zu", g_tables[(a >> 40) - R_TABLE], (size_t)(a & (((uintptr_t)1 << 40) - 1)));
    else
        add(" %s+%zu", names[(a >> 40) - R_SAMPLE], (size_t)(a & (((uintptr_t)1 << 40) - 1)));
}

template <class A>
static void add_arg(A a)
{
    if constexpr (std::is_pointer_v<A>)
        add_ptr((const void *)a);
    else if constexpr (std::is_floating_point_v<A>)
        add(" %.9g", (double)a);
    else
        add(" %llu", (unsigned long long)a);
}

template <auto K>
struct KernelTag {};

/* "mm_chain_fft_kernel<float, 8, 3, 3, true>": the type's name carries the instance (__PRETTY_FUNCTION__ drops its arguments) */
template <auto K>
static std::string kernel_name()
{
    int st = 0;
    char *d = abi::__cxa_demangle(typeid(KernelTag<K>).name(), nullptr, nullptr, &st);
    std::string s = d ? d : typeid(KernelTag<K>).name(); /* "trace::KernelTag<&(void (anonymous namespace)::kernel<args>(params))>" */
    free(d);
    const size_t a = s.find("::mm_");
    if (a == std::string::npos)
        return s;
    size_t b = s.find_first_not_of("abcdefghijklmnopqrstuvwxyz_0123456789", a + 2);
    if (b != std::string::npos && s[b] == '<')
        b = s.find(">(", b) + 1;
    return s.substr(a + 2, b - a - 2);
}

template <auto K, class... A>
static void launch(dim3 g, dim3 b, size_t lds, hipStream_t, A... a)
{
    static const std::string name = kernel_name<K>();
    add(" L %s g=%u,%u,%u b=%u,%u,%u lds=%zu :", name.c_str(), g.x, g.y, g.z, b.x, b.y, b.z, lds);
    (add_arg(a), ...);
    add("\n");
}

static hipError_t table_malloc(void **p, size_t bytes)
{
    *p = region(R_TABLE + (unsigned int)g_tables.size());
    g_tables.push_back(bytes);
    add(" table %zu\n", bytes);
    return hipSuccess;
}

static hipError_t ws_malloc(void **p, size_t bytes)
{
    g_alloc = bytes;
    *p = (void *)kWs;
    return hipSuccess;
}

static hipError_t set_attribute(const void *, hipFuncAttribute attr, int v)
{
    add(" attr %d %d\n", (int)attr, v);
    return hipSuccess;
}

} // namespace trace

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) trace::launch<kernel>(grid, block, lds, stream, ##__VA_ARGS__)
#define hipMalloc(p, bytes) trace::table_malloc((void **)(p), bytes)
#define hipMemcpy(dst, src, bytes, kind) hipSuccess
#define hipFree(p) hipSuccess
#define hipMallocAsync(p, bytes, stream) trace::ws_malloc((void **)(p), bytes)
#define hipFreeAsync(p, stream) hipSuccess
#define hipGetLastError() hipSuccess
#define hipFuncSetAttribute(...) trace::set_attribute(__VA_ARGS__) /* the function's template arguments bring commas */
#define mm_check_device(device) (trace::g_dev_status)

#ifndef MM_STATS_UNIT
#define MM_STATS_UNIT "../../mini_mcmc_amd/csrc/mm_stats.hip"
#endif
#include MM_STATS_UNIT

extern "C" int mmcmc_tracker_within_var(struct mmcmc_tracker *, float *, float *, void *) { return MMCMC_ERR_STATE; }
extern "C" int mmcmc_tracker_shape(struct mmcmc_tracker *, size_t *, size_t *, int *) { return MMCMC_ERR_STATE; }

namespace trace {

/* FIPS 180-4 */
struct Sha256 {
    uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    unsigned char buf[64];
    uint64_t len = 0;
    static uint32_t ror(uint32_t x, int n) { return x >> n | x << (32 - n); }
    void block(const unsigned char *p)
    {
        static const uint32_t k[64] = {
            0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01,
            0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc,
            0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147,
            0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
            0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08,
            0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
            0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
        uint32_t w[64], a[8];
        for (int i = 0; i < 16; ++i)
            w[i] = (uint32_t)p[4 * i] << 24 | (uint32_t)p[4 * i + 1] << 16 | (uint32_t)p[4 * i + 2] << 8 | p[4 * i + 3];
        for (int i = 16; i < 64; ++i)
            w[i] = w[i - 16] + (ror(w[i - 15], 7) ^ ror(w[i - 15], 18) ^ w[i - 15] >> 3) + w[i - 7] +
                   (ror(w[i - 2], 17) ^ ror(w[i - 2], 19) ^ w[i - 2] >> 10);
        memcpy(a, h, sizeof a);
        for (int i = 0; i < 64; ++i) {
            const uint32_t t1 = a[7] + (ror(a[4], 6) ^ ror(a[4], 11) ^ ror(a[4], 25)) + ((a[4] & a[5]) ^ (~a[4] & a[6])) + k[i] + w[i];
            const uint32_t t2 = (ror(a[0], 2) ^ ror(a[0], 13) ^ ror(a[0], 22)) + ((a[0] & a[1]) ^ (a[0] & a[2]) ^ (a[1] & a[2]));
            memmove(a + 1, a, 7 * sizeof a[0]);
            a[4] += t1;
            a[0] = t1 + t2;
        }
        for (int i = 0; i < 8; ++i)
            h[i] += a[i];
    }
    void update(const std::string &s)
    {
        for (unsigned char c : s) {
            buf[len++ % 64] = c;
            if (len % 64 == 0)
                block(buf);
        }
    }
    std::string hex()
    {
        const uint64_t bits = len * 8;
        update(std::string(1, (char)0x80));
        while (len % 64 != 56)
            update(std::string(1, (char)0));
        for (int i = 7; i >= 0; --i)
            update(std::string(1, (char)(bits >> (8 * i))));
        char out[65];
        for (int i = 0; i < 8; ++i)
            snprintf(out + 8 * i, 9, "%08x", h[i]);
        return out;
    }
};

constexpr unsigned int kParts = 16; /* what both entry points ask for */

struct Case {
    int sel, dtype;
    bool aligned, wb;
    size_t C, n, D;
};

/* one call of the internal function */
static std::string run(const Case &c)
{
    g_lines.clear();
    g_dev_status = MMCMC_OK;
    mmcmc_stats_set_kernel(c.sel);
    add("call sel=%d dt=%d al=%d wb=%d C=%zu n=%zu D=%zu\n", c.sel, c.dtype, (int)c.aligned, (int)c.wb, c.C, c.n, c.D);
    const void *sample = region(R_SAMPLE, c.aligned ? 0 : 4);
    float *means = (float *)region(R_MEANS), *ssq = (float *)region(R_SSQ), *acov = (float *)region(R_ACOV);
    /* with wb_part as mmcmc_split_rhat_mean_ess calls it (partial totals and the total in one place), without as
     * mmcmc_stats_partials does (the total goes to the caller's array) */
    double *wb = c.wb ? (double *)region(R_WB) : nullptr;
    float *total = c.wb ? nullptr : (float *)region(R_FINAL);
    /* on a workspace, and once more without one for the size the call allocates itself (no entry point does that today) */
    bool wrote_total = false;
    int st = 0;
    for (float *ws : {(float *)kWs, (float *)nullptr}) {
        const size_t mark = g_lines.size();
        g_alloc = 0;
#ifdef STATS_TRACE_PARENT
        unsigned int parts = 0;
        const int s2 = stats_partials_impl(sample, c.dtype, c.C, c.n, c.D, means, ssq, acov, wb, ws, kParts, 0, nullptr, &parts, total);
        wrote_total = parts != kParts;
#else
        const int s2 = stats_partials_impl(sample, c.dtype, c.C, c.n, c.D, means, ssq, acov, total ? total : acov, wb, ws, kParts, 0,
                                           nullptr, &wrote_total);
#endif
        if (ws)
            st = s2;
        else
            g_lines.resize(mark); /* the same launches again */
        if (s2 != st)
            add(" status without a workspace %d\n", s2);
    }
#ifdef STATS_TRACE_PARENT
    const size_t ws_floats = stats_ws_floats(c.C, c.n, c.D, kParts, 0);
#else
    const size_t ws_floats = mm_stats_ws_floats(c.C, c.n, c.D, kParts, stats_knobs());
#endif
    /* the allocation of a refused call is no part of the record (before the plan, the residue path's 32-bit refusals came
     * after it and left it behind) */
    add(" ret st=%d total=%d ws=%zu alloc=%zu\n", st, (int)(st == MMCMC_OK && wrote_total), ws_floats, st == MMCMC_OK ? g_alloc : (size_t)0);
    return g_lines;
}

static const size_t kM[] = {1,    2,    3,    50,   100,  101,  180,  256,   257,   400,   512,    513,   800,  1024,
                            1025, 1500, 2048, 2049, 2500, 3072, 3073, 8000,  16384, 16385, 65000,  131072, 131073};
static const size_t kD[] = {1, 3, 4, 5, 12, 13, 16, 17, 33, 4097, 65537};
static const size_t kC[] = {1, 2, 3, 9, 1000, 2048, 2049, 65536, (size_t)1 << 26}; /* the last: 2 C D >= 2^31 from D = 16 */

/* every call of half-chain length m, fed to `sink` */
template <class F>
static size_t walk_m(size_t m, F &&sink)
{
    size_t calls = 0;
    for (int sel = MMCMC_STATS_KERNEL_AUTO; sel <= MMCMC_STATS_KERNEL_DIRECT; ++sel)
        for (int dtype : {MMCMC_F32, MMCMC_F64})
            for (bool aligned : {true, false})
                for (bool wb : {true, false})
                    for (size_t n : {2 * m, 2 * m + 1})
                        for (size_t D : kD)
                            for (size_t C : kC) {
                                sink(run(Case{sel, dtype, aligned, wb, C, n, D}));
                                ++calls;
                            }
    /* beyond the direct-work limit (65536 x 3 x m^2 > 2^46 from m = 18919) with the limit at 0, and back at its default */
    if (m >= 65000)
        for (uint64_t limit : {(uint64_t)0, (uint64_t)1 << 46}) {
            mmcmc_stats_set_direct_work_limit(limit);
            for (int dtype : {MMCMC_F32, MMCMC_F64}) {
                sink(run(Case{MMCMC_STATS_KERNEL_DIRECT, dtype, true, true, 65536, 2 * m, 3}));
                ++calls;
            }
        }
    return calls;
}

/* the two public entry points up to the device check (answered MMCMC_ERR_NO_DEVICE here): the statuses of bad arguments and
 * bad shapes, which come before it */
template <class F>
static size_t walk_entry(F &&sink)
{
    size_t calls = 0;
    g_dev_status = MMCMC_ERR_NO_DEVICE;
    float *out = (float *)region(R_ACOV);
    for (bool sample : {false, true})
        for (bool outs : {false, true})
            for (int dtype : {MMCMC_F32, MMCMC_F64, 7})
                for (size_t C : {(size_t)0, (size_t)1, (size_t)2})
                    for (size_t D : {(size_t)0, (size_t)1, (size_t)8191, (size_t)8192, (size_t)32768, (size_t)65535, (size_t)65536})
                        for (size_t n : {(size_t)0, (size_t)1, (size_t)2, (size_t)3, (size_t)2049, (size_t)2050, (size_t)262144,
                                         (size_t)262145, (size_t)262146, ((size_t)1 << 31) - 1, (size_t)1 << 31}) {
                            g_lines.clear();
                            const void *s = sample ? region(R_SAMPLE) : nullptr;
                            float *o = outs ? out : nullptr;
                            const int a = mmcmc_stats_partials(s, dtype, C, n, D, o, o, o, 0, nullptr);
                            const int b = mmcmc_split_rhat_mean_ess(s, 1, dtype, C, n, D, o, o, 0, nullptr);
                            add("entry sample=%d out=%d dt=%d C=%zu n=%zu D=%zu partials=%d split_rhat=%d\n", (int)sample, (int)outs,
                                dtype, C, n, D, a, b);
                            sink(g_lines);
                            calls += 2;
                        }
    return calls;
}

struct Named {
    const char *name;
    Case c;
    uint64_t limit;
};
constexpr uint64_t kLimit = (uint64_t)1 << 46;
/* the benchmark's shape, the first and the last shape of each path, each refusal */
static const Named kNamed[] = {
    {"benchmark [65536, 400, 3] f32", {0, 0, true, true, 65536, 400, 3}, kLimit},
    {"benchmark shape through mmcmc_stats_partials", {0, 0, true, false, 65536, 400, 3}, kLimit},
    {"tile1 first: m = 1", {0, 0, true, true, 9, 2, 1}, kLimit},
    {"tile1 last under auto: m = 100", {0, 0, true, true, 65536, 201, 3}, kLimit},
    {"tile1 NPRE = 8: m = 257 forced", {2, 0, true, true, 65536, 514, 3}, kLimit},
    {"tile1 last: m = 512 forced", {2, 1, true, true, 65536, 1024, 4}, kLimit},
    {"tile1 asked for, parts x dim > slabs: tile", {2, 0, true, true, 1, 400, 3}, kLimit},
    {"tile, 16-byte loads", {3, 0, true, true, 2048, 200, 4}, kLimit},
    {"tile, unaligned sample", {3, 0, false, true, 2048, 200, 4}, kLimit},
    {"tile f64, 8 tiles per lane", {3, 1, true, true, 2049, 400, 3}, kLimit},
    {"tile asked for, too many tiles: MFMA", {3, 0, true, true, 1000, 1024, 3}, kLimit},
    {"MFMA first: m = 1", {4, 0, true, true, 1000, 2, 1}, kLimit},
    {"MFMA, dim 13", {4, 0, true, true, 1000, 200, 13}, kLimit},
    {"MFMA asked for, LDS too small: half-chain", {4, 0, true, true, 1000, 2048, 12}, kLimit},
    {"half-chain in LDS, limit raised", {5, 0, true, true, 1000, 4096, 5}, kLimit},
    {"half-chain in LDS last: m = 16384", {5, 1, true, true, 9, 32768, 1}, kLimit},
    {"any-length first: m = 16385", {5, 0, true, true, 9, 32770, 1}, kLimit},
    {"any-length: dim 4097 at m = 3", {5, 0, true, true, 9, 6, 4097}, kLimit},
    {"short transform first under auto: m = 101", {0, 0, true, true, 65536, 202, 3}, kLimit},
    {"short transform first forced: m = 2", {1, 0, true, true, 65536, 4, 3}, kLimit},
    {"short transform R1 = 8 last: m = 256", {0, 0, true, true, 65536, 512, 4}, kLimit},
    {"short transform R1 = 16: m = 257, dim 5", {0, 1, true, true, 1000, 514, 5}, kLimit},
    {"short transform R1 = 32 last: m = 1024", {0, 0, true, false, 65536, 2049, 3}, kLimit},
    {"short transform, few chains", {0, 0, true, true, 3, 400, 17}, kLimit},
    {"long transform N1 = 2 first: m = 1025", {0, 0, true, true, 65536, 2050, 3}, kLimit},
    {"long transform N1 = 2 last: m = 2048", {0, 1, true, false, 2049, 4096, 33}, kLimit},
    {"residues first: m = 2049, means kernel", {0, 0, true, true, 65536, 4098, 3}, kLimit},
    {"residues, dim 17: moments kernel", {0, 0, true, true, 1000, 6144, 17}, kLimit},
    {"residues last: m = 131072", {0, 0, true, true, 2, 262144, 1}, kLimit},
    {"beyond the transforms under auto: any-length", {0, 0, true, true, 2, 262146, 1}, kLimit},
    {"refused: dim 65537", {0, 0, true, true, 9, 400, 65537}, kLimit},
    {"refused: n = 1", {0, 0, true, true, 9, 1, 3}, kLimit},
    {"refused: bins beyond 32 bits", {5, 0, true, true, 1, 262144, 16384}, kLimit},
    {"refused: residues, 2 C D >= 2^31", {0, 0, true, true, (size_t)1 << 26, 4098, 17}, kLimit},
    {"refused: any-length, 2 C D >= 2^31", {5, 0, true, true, (size_t)1 << 26, 32770, 16}, kLimit},
    {"refused: any-length, dim x m >= 2^32", {5, 0, true, true, 1, 2097152, 4097}, kLimit},
    {"refused: direct work beyond the limit", {5, 0, true, true, 65536, 262146, 3}, kLimit},
    {"the same with the limit at 0", {5, 0, true, true, 65536, 262146, 3}, 0},
    {"refused: dtype 7", {0, 7, true, true, 9, 400, 3}, kLimit},
    {"refused: no chains", {0, 0, true, true, 0, 400, 3}, kLimit},
};

} // namespace trace

int main(int argc, char **argv)
{
    using namespace trace;
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "--named") {
        for (const Named &nc : kNamed) {
            mmcmc_stats_set_direct_work_limit(nc.limit);
            printf("# %s\n%s", nc.name, run(nc.c).c_str());
        }
        return 0;
    }
    if (mode == "--lines" && argc > 2) {
        auto print = [](const std::string &s) { fputs(s.c_str(), stdout); };
        if (!strcmp(argv[2], "entry"))
            walk_entry(print);
        else
            walk_m((size_t)strtoull(argv[2], nullptr, 10), print);
        return 0;
    }
    size_t calls = 0;
    for (size_t m : kM) {
        Sha256 sha;
        const size_t k = walk_m(m, [&](const std::string &s) { sha.update(s); });
        printf("m %zu calls %zu sha256 %s\n", m, k, sha.hex().c_str());
        calls += k;
    }
    Sha256 sha;
    const size_t k = walk_entry([&](const std::string &s) { sha.update(s); });
    printf("entry calls %zu sha256 %s\n", k, sha.hex().c_str());
    printf("calls %zu\n", calls + k);
    return 0;
}
