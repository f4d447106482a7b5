// The engine's scalar math (csrc/mm_math.h, mm_accept_stat of csrc/mm_nuts.h, mm_box_muller_f64 of csrc/mm_rng.h) evaluated ON THE
// DEVICE over an input list that tests/test_math_specials.py writes; compiled and run by that test on the GPU box.
//   input file:  seven uint64 counts (e32, e64, l32, l64, u32, u64, b64), then the arrays in that order:
//                e32 floats / e64 doubles   arguments of the exponentials and of mm_accept_stat
//                l32 floats / l64 doubles   arguments of the logarithms (positive, normal)
//                u32 floats / u64 doubles   u in [0, 1] for sin / cos (2 pi u)
//                b64 pairs of doubles       (u1, u2) of the Box-Muller transform
//   stdout:      one line per result array, "<name> <count> <hex words>", 8 hex digits per f32 and 16 per f64 result
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mm_nuts.h"

#define CHECK(e)                                                                          \
    do {                                                                                  \
        hipError_t e_ = (e);                                                              \
        if (e_ != hipSuccess) {                                                           \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(e_));    \
            return 2;                                                                     \
        }                                                                                 \
    } while (0)

// mm_expf_sel / mm_exp_sel exist in the device pass only; the host pass merely parses the functors
#if defined(__HIP_DEVICE_COMPILE__)
#define SEL32(x) mm_expf_sel(x)
#define SEL64(x) mm_exp_sel(x)
#else
#define SEL32(x) (x)
#define SEL64(x) (x)
#endif

struct f_expf { __device__ void operator()(const float *x, float *o) const { o[0] = mm_expf(x[0]); } };
struct f_expf_sel { __device__ void operator()(const float *x, float *o) const { o[0] = SEL32(x[0]); } };
struct f_acc32 { __device__ void operator()(const float *x, float *o) const { o[0] = mm_accept_stat<float>(x[0]); } };
struct f_logf { __device__ void operator()(const float *x, float *o) const { o[0] = mm_logf(x[0]); } };
struct f_sc32 { __device__ void operator()(const float *x, float *o) const { mm_sincos2pif(x[0], &o[0], &o[1]); } };
struct f_exp { __device__ void operator()(const double *x, double *o) const { o[0] = mm_exp(x[0]); } };
struct f_exp_sel { __device__ void operator()(const double *x, double *o) const { o[0] = SEL64(x[0]); } };
struct f_acc64 { __device__ void operator()(const double *x, double *o) const { o[0] = mm_accept_stat<double>(x[0]); } };
struct f_log { __device__ void operator()(const double *x, double *o) const { o[0] = mm_log(x[0]); } };
struct f_sc64 { __device__ void operator()(const double *x, double *o) const { mm_sincos2pi(x[0], &o[0], &o[1]); } };
struct f_bm64 { __device__ void operator()(const double *x, double *o) const { mm_box_muller_f64(x[0], x[1], &o[0], &o[1]); } };

// element i: NIN inputs at in[i * NIN], NOUT results at out[i * NOUT]
template <class T, int NIN, int NOUT, class F> __global__ void apply(const T *in, T *out, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        F()(in + i * NIN, out + i * NOUT);
}

template <class T, int NIN, int NOUT, class F> static int run(const char *name, const std::vector<T> &in)
{
    const size_t n = in.size() / NIN;
    std::vector<T> out(n * NOUT);
    if (n) {
        T *d_in = nullptr, *d_out = nullptr;
        CHECK(hipMalloc((void **)&d_in, in.size() * sizeof(T)));
        CHECK(hipMalloc((void **)&d_out, out.size() * sizeof(T)));
        CHECK(hipMemcpy(d_in, in.data(), in.size() * sizeof(T), hipMemcpyHostToDevice));
        hipLaunchKernelGGL((apply<T, NIN, NOUT, F>), dim3((unsigned int)((n + 255) / 256)), dim3(256), 0, 0, d_in, d_out, n);
        CHECK(hipGetLastError());
        CHECK(hipMemcpy(out.data(), d_out, out.size() * sizeof(T), hipMemcpyDeviceToHost));
        CHECK(hipFree(d_in));
        CHECK(hipFree(d_out));
    }
    printf("%s %zu ", name, out.size());
    for (const T &v : out) {
        if (sizeof(T) == 4) {
            uint32_t w;
            memcpy(&w, &v, 4);
            printf("%08x", w);
        } else {
            uint64_t w;
            memcpy(&w, &v, 8);
            printf("%016llx", (unsigned long long)w);
        }
    }
    printf("\n");
    return 0;
}

template <class T> static bool read_vec(FILE *f, size_t n, std::vector<T> &v)
{
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: %s <input file>\n", argv[0]);
        return 1;
    }
    FILE *f = fopen(argv[1], "rb");
    uint64_t cnt[7];
    if (!f || fread(cnt, sizeof(uint64_t), 7, f) != 7) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 1;
    }
    for (uint64_t c : cnt)
        if (c > (1ull << 24)) {
            fprintf(stderr, "count %llu out of range\n", (unsigned long long)c);
            return 1;
        }
    std::vector<float> e32, l32, u32;
    std::vector<double> e64, l64, u64, b64;
    if (!read_vec(f, cnt[0], e32) || !read_vec(f, cnt[1], e64) || !read_vec(f, cnt[2], l32) || !read_vec(f, cnt[3], l64) ||
        !read_vec(f, cnt[4], u32) || !read_vec(f, cnt[5], u64) || !read_vec(f, 2 * cnt[6], b64)) {
        fprintf(stderr, "short input file\n");
        return 1;
    }
    fclose(f);
    int rc = 0;
    rc |= run<float, 1, 1, f_expf>("expf", e32);
    rc |= run<float, 1, 1, f_expf_sel>("expf_sel", e32);
    rc |= run<float, 1, 1, f_acc32>("accept32", e32);
    rc |= run<double, 1, 1, f_exp>("exp", e64);
    rc |= run<double, 1, 1, f_exp_sel>("exp_sel", e64);
    rc |= run<double, 1, 1, f_acc64>("accept64", e64);
    rc |= run<float, 1, 1, f_logf>("logf", l32);
    rc |= run<double, 1, 1, f_log>("log", l64);
    rc |= run<float, 1, 2, f_sc32>("sincos32", u32);
    rc |= run<double, 1, 2, f_sc64>("sincos64", u64);
    rc |= run<double, 2, 2, f_bm64>("boxmuller", b64);
    return rc;
}
