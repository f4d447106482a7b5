// White-box probe of the running-diagnostics tracker (csrc/mm_tracker.hip), compiled and run by
// tests/test_tracker_edges.py on the GPU box with the flags of csrc/Makefile (and once more with -DMMCMC_TUNING, run with
// MMCMC_TRACKER_ONE_WAVE=1, which reaches tracker_step_tiled_kernel<T, D> for D > 1).
//
// It includes the unit itself, so it sees struct mmcmc_tracker and needs no libmmcmc.so, and it drives the public entry
// points only: mmcmc_tracker_create, optionally mmcmc_tracker_init_last, then a list of mmcmc_tracker_steps calls.  After
// every steps call it copies back what the C ABI never shows -- the per-chain mean, mean of squares, last state and
// acceptance average, the k x C flag bytes of the call, and p_accept -- and at the end of a case the results of
// mmcmc_tracker_stats, _chain_stats and _within_var.
//
//   tracker_probe <cases.bin> <out.bin>            (little-endian, written / read by tests/test_tracker_edges.py)
//
//   cases.bin  u32 magic 'TRKP', u32 n_cases, then per case
//                u32 name_len, name; u64 C, D, n_rows; u32 dtype (0 f32, 1 f64), has_init, n_calls;
//                n_calls x (u64 t0, u64 k, u32 states_is_device);
//                [C, D] init (if has_init) and [C, n_rows, D] states, both of dtype
//   out.bin    per case and call: f32 mean[C D], mean_sq[C D], last[C D], p_chain[C]; u8 flags[k C]; f32 p_accept
//              per case: i32 status, f32 rhat[D], max_rhat, p_accept                      (mmcmc_tracker_stats)
//                        i32 status, f32 rhat[D], max_rhat, mean p_accept of the chains   (mmcmc_tracker_chain_stats)
//                        i32 status, f32 within[D], var[D]                                (mmcmc_tracker_within_var)
//                        u64 n
//
// All cases run in one process; every status is checked; the first failure prints the case's name and ends the program
// with a non-zero exit code before anything else is launched.
#include "../../mini_mcmc_amd/csrc/mm_tracker.hip"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>

namespace {

std::string g_case = "(reading the header)";

[[noreturn]] void fail(const char *what, long code)
{
    std::fprintf(stderr, "tracker_probe: case %s: %s failed (%ld)\n", g_case.c_str(), what, code);
    std::fflush(stderr);
    std::_Exit(1);
}

#define PROBE_HIP(expr)                                                                                              \
    do {                                                                                                             \
        hipError_t e_ = (expr);                                                                                      \
        if (e_ != hipSuccess) {                                                                                      \
            std::fprintf(stderr, "  %s\n", hipGetErrorString(e_));                                                   \
            fail(#expr, (long)e_);                                                                                   \
        }                                                                                                            \
    } while (0)

#define PROBE_OK(expr)                                                                                               \
    do {                                                                                                             \
        int s_ = (expr);                                                                                             \
        if (s_ != MMCMC_OK)                                                                                          \
            fail(#expr, (long)s_);                                                                                   \
    } while (0)

void get(std::FILE *f, void *dst, size_t bytes)
{
    if (bytes && std::fread(dst, 1, bytes, f) != bytes)
        fail("reading the case file", (long)bytes);
}

template <class V>
V get(std::FILE *f)
{
    V v;
    get(f, &v, sizeof v);
    return v;
}

void put(std::FILE *f, const void *src, size_t bytes)
{
    if (bytes && std::fwrite(src, 1, bytes, f) != bytes)
        fail("writing the result file", (long)bytes);
}

struct Call {
    uint64_t t0, k;
    uint32_t is_device;
};

} // namespace

int main(int argc, char **argv)
{
    if (argc != 3) {
        std::fprintf(stderr, "usage: tracker_probe <cases.bin> <out.bin>\n");
        return 2;
    }
    std::FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out)
        fail("opening the files", 0);
    if (get<uint32_t>(in) != 0x504b5254u) /* "TRKP" */
        fail("the magic number", 0);
    const uint32_t n_cases = get<uint32_t>(in);
    for (uint32_t ic = 0; ic < n_cases; ++ic) {
        const uint32_t name_len = get<uint32_t>(in);
        if (name_len > 256)
            fail("the length of the next case's name", (long)name_len);
        std::string name(name_len, '\0');
        get(in, &name[0], name_len);
        g_case = name;
        const uint64_t C = get<uint64_t>(in), D = get<uint64_t>(in), n_rows = get<uint64_t>(in);
        const uint32_t dtype = get<uint32_t>(in), has_init = get<uint32_t>(in), n_calls = get<uint32_t>(in);
        if (C < 2 || C > (1u << 20) || D == 0 || D > 64 || n_rows == 0 || n_rows > 4096 || dtype > 1 || n_calls == 0 ||
            n_calls > 4096)
            fail("the shape of the case", (long)ic);
        std::vector<Call> calls(n_calls);
        for (Call &c : calls) {
            c.t0 = get<uint64_t>(in);
            c.k = get<uint64_t>(in);
            c.is_device = get<uint32_t>(in);
            if (c.k == 0 || c.t0 + c.k > n_rows)
                fail("the rows of a call", (long)c.t0);
        }
        const size_t esz = dtype == MMCMC_F32 ? 4 : 8, cd = C * D;
        std::vector<char> init(has_init ? cd * esz : 0), states(C * n_rows * D * esz);
        get(in, init.data(), init.size());
        get(in, states.data(), states.size());

        void *d_states = nullptr;
        PROBE_HIP(hipMalloc(&d_states, states.size()));
        PROBE_HIP(hipMemcpy(d_states, states.data(), states.size(), hipMemcpyHostToDevice));
        mmcmc_tracker *h = nullptr;
        PROBE_OK(mmcmc_tracker_create(&h, C, D, 0));
        if (has_init)
            PROBE_OK(mmcmc_tracker_init_last(h, init.data(), 0, (int)dtype, nullptr));
        std::vector<float> buf(3 * cd + C);
        std::vector<unsigned char> flags;
        for (const Call &c : calls) {
            PROBE_OK(mmcmc_tracker_steps(h, c.is_device ? d_states : (const void *)states.data(), (int)c.is_device, (int)dtype,
                                         n_rows, c.t0, c.k, nullptr));
            PROBE_HIP(hipDeviceSynchronize());
            if (h->flags_cap < c.k * C)
                fail("the capacity of the flags", (long)h->flags_cap);
            flags.resize(c.k * C);
            float p = 0.f;
            PROBE_HIP(hipMemcpy(buf.data(), h->d_mean, cd * 4, hipMemcpyDeviceToHost));
            PROBE_HIP(hipMemcpy(buf.data() + cd, h->d_mean_sq, cd * 4, hipMemcpyDeviceToHost));
            PROBE_HIP(hipMemcpy(buf.data() + 2 * cd, h->d_last, cd * 4, hipMemcpyDeviceToHost));
            PROBE_HIP(hipMemcpy(buf.data() + 3 * cd, h->d_p_chain, C * 4, hipMemcpyDeviceToHost));
            PROBE_HIP(hipMemcpy(flags.data(), h->d_flags, flags.size(), hipMemcpyDeviceToHost));
            PROBE_HIP(hipMemcpy(&p, h->d_p, 4, hipMemcpyDeviceToHost));
            put(out, buf.data(), buf.size() * 4);
            put(out, flags.data(), flags.size());
            put(out, &p, 4);
        }
        /* the aggregates; before the second step they answer MMCMC_ERR_STATE, which is recorded, not a failure */
        auto agg_status = [&](const char *what, int s) -> int32_t {
            if (s != MMCMC_OK && !(s == MMCMC_ERR_STATE && h->n < 2))
                fail(what, (long)s);
            return (int32_t)s;
        };
        std::vector<float> r(2 * D + 2, 0.f);
        int32_t s = agg_status("mmcmc_tracker_stats", mmcmc_tracker_stats(h, r.data(), &r[D], &r[D + 1], nullptr));
        put(out, &s, 4);
        put(out, r.data(), (D + 2) * 4);
        r.assign(2 * D + 2, 0.f);
        s = agg_status("mmcmc_tracker_chain_stats", mmcmc_tracker_chain_stats(h, r.data(), &r[D], &r[D + 1], nullptr));
        put(out, &s, 4);
        put(out, r.data(), (D + 2) * 4);
        r.assign(2 * D + 2, 0.f);
        s = agg_status("mmcmc_tracker_within_var", mmcmc_tracker_within_var(h, r.data(), r.data() + D, nullptr));
        put(out, &s, 4);
        put(out, r.data(), 2 * D * 4);
        const uint64_t n = h->n;
        put(out, &n, 8);
        PROBE_HIP(hipDeviceSynchronize());
        PROBE_OK(mmcmc_tracker_destroy(h));
        PROBE_HIP(hipFree(d_states));
    }
    g_case = "(closing)";
    if (std::fclose(out) != 0)
        fail("closing the result file", 0);
    std::fclose(in);
    std::printf("tracker_probe: %u cases\n", n_cases);
    return 0;
}
